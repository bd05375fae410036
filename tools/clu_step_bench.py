"""What one host clustering step costs: a loop over `dz_clu_step` alone, no GPU.

One stream of `--steps` chunks with K local speakers, D-dimensional embeddings and G centroids (3, 512 and 20 by default:
`pyannote/embedding` in the default pipeline), voices from a pool a little larger than G, NaN embeddings, duplicated rows
and silent chunks mixed in as in tests/test_clustering.py.  The inputs are drawn first; the timed loop only calls the
library through ctypes.  `--lib` names the shared library to load (default: this tree's), so that two builds can be run
in turn; `--runs` repeats the loop on a fresh handle.  One JSON line: microseconds per step of every run, their median,
and a digest of the assignments (the same for two builds that decide the same)."""
import argparse
import ctypes as C
import hashlib
import json
import statistics
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--lib", type=str, default=str(ROOT / "diart_amd" / "libdiart_amd.so"))
    ap.add_argument("--steps", type=int, default=4000)
    ap.add_argument("--runs", type=int, default=1)
    ap.add_argument("--frames", type=int, default=293)
    ap.add_argument("-K", type=int, default=3)
    ap.add_argument("-D", type=int, default=512)
    ap.add_argument("-G", type=int, default=20)
    args = ap.parse_args()
    T, F, K, D, G = args.steps, args.frames, args.K, args.D, args.G
    rng = np.random.default_rng(0)
    pool = rng.standard_normal((G + 6, D))
    seg = (rng.random((T, F, K)) * (rng.random((T, 1, K)) < 0.8) * rng.choice([0.3, 0.8, 1.0], (T, 1, K))).astype(np.float32)
    emb = np.empty((T, K, D), dtype=np.float32)
    for t in range(T):
        e = pool[rng.choice(len(pool), K, replace=False)] + 0.4 * rng.standard_normal((K, D))
        emb[t] = e / np.linalg.norm(e, axis=1, keepdims=True)
        r = rng.random()
        if r < 0.05:
            emb[t, rng.integers(K)] = np.nan
        elif r < 0.1 and K > 1:
            emb[t, 1] = emb[t, 0]
        elif r < 0.13:
            seg[t] = 0
    lib = C.CDLL(args.lib)
    lib.dz_clu_create.argtypes = [C.c_double, C.c_double, C.c_double, C.c_int, C.POINTER(C.c_void_p)]
    lib.dz_clu_step.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.dz_clu_destroy.argtypes = [C.c_void_p]
    scores = np.empty((F, G), dtype=np.float64)
    assign = np.full((T, K), -1, dtype=np.int32)      # a step that raises leaves its row
    sp, ep, ap_ = seg.ctypes.data, emb.ctypes.data, assign.ctypes.data
    s_stride, e_stride, a_stride = F * K * 4, K * D * 4, K * 4
    us, raised = [], 0
    for _ in range(args.runs):
        h = C.c_void_p()
        assert lib.dz_clu_create(0.55, 0.25, 1.057, G, C.byref(h)) == 0
        step, out = lib.dz_clu_step, scores.ctypes.data
        raised = 0
        t0 = time.perf_counter()
        for t in range(T):
            raised += step(h, sp + t * s_stride, F, K, ep + t * e_stride, D, out, ap_ + t * a_stride) != 0
        us.append(1e6 * (time.perf_counter() - t0) / T)
        lib.dz_clu_destroy(h)
    print(json.dumps(dict(tool="tools/clu_step_bench.py", lib=args.lib, steps=T, frames=F, K=K, D=D, G=G,
                          us_per_step=[round(u, 3) for u in us], us_per_step_median=round(statistics.median(us), 3),
                          steps_that_raise=int(raised), assign_sha256=hashlib.sha256(assign.tobytes()).hexdigest()[:16])))


if __name__ == "__main__":
    main()
