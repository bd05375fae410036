"""The crafted cache of the whole-file diarization tests (tests/test_offline_host.py, tests/test_gpu_offline.py): three
speakers over 40 chunks of 59 frames and 3 local speakers, with the corners the reconstruction has to get right."""
import numpy as np

C, F, K, D = 40, 59, 3, 64
HOP = 5                      # output frames between two chunks
RES, STEP = 0.1, 0.5
TAU = 0.6
NAN_CHUNK, TWIN_CHUNK = 17, 5
SPANS = ((0, 100), (70, 170), (140, 254))        # output frames in which each speaker talks


def crafted_file(seed=3):
    """seg (C, F, K) float32, emb (C, K, D) float32, starts (C,): speakers 0 and 1 overlap in frames 70 .. 99, where even
    chunks hear both and odd chunks hear one (mean count x.5 where as many even as odd chunks cover a frame); speakers 1
    and 2 overlap in 140 .. 169, where even chunks hear both at the same score and odd chunks neither (count 1, equal
    A); chunk NAN_CHUNK is all NaN; in chunk TWIN_CHUNK two local speakers carry the same voice."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((3, D))
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    seg = np.full((C, F, K), 0.05, dtype=np.float32)
    emb = np.zeros((C, K, D), dtype=np.float32)
    for c in range(C):
        perm = rng.permutation(K)
        t = HOP * c + np.arange(F)
        talks = [(t >= a) & (t < b) for a, b in SPANS]
        for g in range(3):
            level = np.full(F, 0.9, dtype=np.float32)
            if c % 2:
                if g == 1:
                    level[talks[0]] = 0.3            # odd chunks hear only speaker 0 where 0 and 1 overlap
                if g in (1, 2):
                    level[talks[1] & talks[2]] = 0.3     # and neither of 1 and 2 where those overlap
            seg[c, talks[g], perm[g]] = level[talks[g]]
            emb[c, perm[g]] = (centres[g] + 0.05 * rng.standard_normal(D)) * rng.uniform(0.5, 2.0)
        if c == TWIN_CHUNK:                         # frames 25 .. 83: speaker 0 alone until 70; split it over two locals
            a, b = perm[0], perm[2]
            seg[c, 30:, b] = seg[c, 30:, a]
            seg[c, 30:, a] = 0.05
            emb[c, b] = (centres[0] + 0.05 * rng.standard_normal(D)) * 1.5
    seg[NAN_CHUNK] = np.nan
    return dict(uri="crafted", seg=seg, emb=emb, starts=STEP * np.arange(C), res=RES, shift=-0.25, reference=[])


def config(max_speakers=20, tau_active=TAU):
    return dict(step=STEP, latency=STEP, tau_active=tau_active, rho_update=0.3, delta_new=1.0, max_speakers=max_speakers)
