"""Weighted statistics pooling (pyannote StatsPool, paper Eq. 1) restated in float64, the measure its kernels are held
to, and the cases of tests/test_gpu_pool_f64.py.  Plain torch; nothing of the product is imported.

The operation, per (chunk, speaker, channel), over the chunk's first T frames x_t with the speaker's weights w_t
(resampled to T frames first, see ``resample``):

    v1 = sum w          v2 = sum w^2
    mean = sum w x / v1
    std  = sqrt( sum w (x - mean)^2 / (v1 - v2 / v1) )

The measure.  A max-over-the-tensor bound hides a wrong channel behind a loud one and a wrong std behind a large mean,
so every element is scaled by what float arithmetic can resolve THERE.  With den = sum w |x| / v1 (the weighted mean
magnitude of what was summed) and kappa = v1 / (v1 - v2 / v1) (1 / (1 - 1 / n_eff): how much of v1 the denominator's
subtraction cancels):

    err_mean = |got - ref| / den
    err_std  = |got - ref| / (kappa * std_ref + sqrt(kappa) * den)

Why these denominators.  A backward-stable weighted sum has |d mean| <= c eps den, whatever cancels between the
terms: err_mean is in units of eps.  For the std, write var = S / D with S = sum w (x - mean)^2, D = v1 - v2 / v1.
 (a) D.  v1 and v2 / v1 each carry a relative error of some eps; their difference D therefore carries a RELATIVE error
     of kappa eps, var the same, std half of it: |d std| <= kappa eps std.  First term.
 (b) S.  A two-pass algorithm centres on its own computed mean m' = mean + dm.  sum w (x - m')^2 = S + v1 dm^2 exactly
     (the cross term vanishes at the true mean), so the mean's error enters the variance only as dm^2 v1 / D = kappa dm^2
     and |d std| <= sqrt(kappa) |dm| even when std -> 0; the rounding of the terms themselves, eps (|x| + |mean|)^2
     relative to S, is of the same form.  With |dm| <= eps den: second term.
A one-pass variance (sum w x^2 - (sum w x)^2 / v1) instead loses eps den^2 / std^2 RELATIVE, which this measure shows
at full size on features far from zero; a biased denominator (v1 for D) is wrong by sqrt(kappa) in std, far beyond
kappa eps.

The gate, one for both halves and both device paths: max(1e-6, 4 e32), e32 the same measure of the float32
restatement (these formulas in torch.float32 on the CPU) on the same case — measured against the reference, never
against a device.  tests/test_pool_ref_host.py holds e32 under 2e-5 in every cell and shows that each planted fault
(``pool_faulty``) exceeds the gate.

Degenerate rows — a condition on the weights, not a measurement.  A (chunk, speaker) row with fewer than two non-zero
resampled weights has D = 0 up to one rounding: no std is defined (``Ref.std_ok`` is False there: compare the mean only,
the device std must be NaN or 0).  A row with no weight at all is 0 / 0 in both halves (``Ref.mean_ok`` False: NaN on
the device).  Nothing else is excluded.
"""
import functools
import math

import torch

F64, F32 = torch.float64, torch.float32
TINY = 1e-30                     # den is clamped here: a column that is exactly 0 on every weighted frame must pool to exactly 0
GATE_FLOOR, GATE_FACTOR = 1e-6, 4.0
E32_CAP = 2e-5                   # tests/test_pool_ref_host.py: no cell's float32 error leaves this
TILE = 128                       # rows of a GEMM tile of the pooled epilogue


def gate(e32):
    return max(GATE_FLOOR, GATE_FACTOR * e32)


# --------------------------------------------------------------------------- weight resampling (torch's index rules)
def nearest_index(F, T):
    """source index of target frame t under F.interpolate(mode="nearest"): min(floor(t * (float32(F) / float32(T))), F - 1),
    the product in float32 as well"""
    scale = torch.tensor(float(F), dtype=F32) / torch.tensor(float(T), dtype=F32)
    return torch.clamp(torch.floor(torch.arange(T, dtype=F32) * scale).long(), max=F - 1)


def linear_taps(F, T, dtype=F64):
    """(i0, i1, l1) of F.interpolate(mode="linear", align_corners=False): src = (F / T) (t + 0.5) - 0.5 clamped at 0,
    i0 = floor(src), i1 = i0 + 1 while inside, l1 = src - i0; out = (1 - l1) w[i0] + l1 w[i1].  All in `dtype`."""
    scale = torch.tensor(float(F), dtype=dtype) / torch.tensor(float(T), dtype=dtype)
    src = torch.clamp(scale * (torch.arange(T, dtype=dtype) + 0.5) - 0.5, min=0.0)
    i0 = src.long()
    i1 = i0 + (i0 < F - 1).long()
    return i0, i1, src - i0.to(dtype)


def resample(w, T, mode, dtype=F64):
    """(rows, F) weights -> (rows, T) in `dtype`; F == T is the identity whatever the mode"""
    w = w.to(dtype)
    Fw = w.shape[1]
    if Fw == T:
        return w
    if mode == "nearest":
        return w[:, nearest_index(Fw, T)]
    assert mode == "linear", mode
    i0, i1, l1 = linear_taps(Fw, T, dtype)
    return (1.0 - l1) * w[:, i0] + l1 * w[:, i1]


# --------------------------------------------------------------------------- pooling
def _moments(x, w, K, dtype):
    xk = x.to(dtype).repeat_interleave(K, dim=0)                    # (rows, T, C)
    w = torch.ones(xk.shape[:2], dtype=dtype) if w is None else w.to(dtype)
    return xk, w, w.sum(1), (w * w).sum(1)


def pool(x, w, K, dtype=F64):
    """x (nx, T, C) features, w (nx * K, T) resampled weights (speaker-major per chunk) or None -> mean, std (nx * K, C)"""
    xk, w, v1, v2 = _moments(x, w, K, dtype)
    mean = (w[:, :, None] * xk).sum(1) / v1[:, None]
    var = (w[:, :, None] * (xk - mean[:, None, :]) ** 2).sum(1) / (v1 - v2 / v1)[:, None]
    return mean, torch.sqrt(var)


class Ref:
    """the float64 pooling of one case with the per-element scales of the measure"""

    def __init__(self, x, w, K, feature_den=None):
        xk, wd, v1, v2 = _moments(x, w, K, F64)
        self.mean, self.std = pool(x, w, K, F64)
        mag = xk.abs() if feature_den is None else feature_den.to(F64).repeat_interleave(K, dim=0)
        self.den = torch.clamp((wd[:, :, None] * mag).sum(1) / v1[:, None], min=TINY)
        nz = (wd != 0).sum(1)
        self.mean_ok, self.std_ok = nz >= 1, nz >= 2
        self.kappa = (v1 / (v1 - v2 / v1))[:, None]
        self.std_scale = self.kappa * self.std + torch.sqrt(self.kappa) * self.den

    def errors(self, mean, std):
        """-> (max err_mean, max err_std) over every element that is not excluded"""
        em = ((mean.to(F64) - self.mean).abs() / self.den)[self.mean_ok]
        es = ((std.to(F64) - self.std).abs() / self.std_scale)[self.std_ok]
        worst = lambda e: float("nan") if torch.isnan(e).any() else (e.max().item() if e.numel() else 0.0)
        return worst(em), worst(es)

    def between(self, a, b):
        """the same measure of the difference of two results"""
        em = ((a[0].to(F64) - b[0].to(F64)).abs() / self.den)[self.mean_ok]
        es = ((a[1].to(F64) - b[1].to(F64)).abs() / self.std_scale)[self.std_ok]
        worst = lambda e: float("nan") if torch.isnan(e).any() else (e.max().item() if e.numel() else 0.0)
        return worst(em), worst(es)

    def e32(self, x, w32, K):
        """the measure of the float32 restatement: w32 = the weights resampled in float32"""
        return max(self.errors(*pool(x, w32, K, F32)))


# --------------------------------------------------------------------------- planted faults (float32, for the host test)
def pool_faulty(fault, xfull, w, K, T, mode):
    """The float32 restatement with one fault planted.  xfull (nx, P, C): the chunks at their pitch, frames T .. P-1
    included; w (nx * K, Fw) source weights or None.  -> mean, std as ``pool``."""
    nx, P, _ = xfull.shape
    x = xfull[:, :T]
    wr = None if w is None else resample(w, T, mode, F32)
    if fault == "biased_denominator":                 # v1 in place of v1 - v2 / v1
        xk, wd, v1, v2 = _moments(x, wr, K, F32)
        mean = (wd[:, :, None] * xk).sum(1) / v1[:, None]
        return mean, torch.sqrt((wd[:, :, None] * (xk - mean[:, None, :]) ** 2).sum(1) / v1[:, None])
    if fault == "boundary_frame":                     # local row rb of a straddling tile goes to the chunk before it:
        # frame 0 of chunk b + 1 (with its own weight) is pooled into chunk b and missing from chunk b + 1
        wd = torch.ones(nx * K, T, dtype=F32) if wr is None else wr
        wd = wd.view(nx, K, T)
        xe = torch.cat([x, torch.cat([x[1:, :1], x[:1, :1]], 0)], 1)                     # (nx, T + 1, C)
        extra = torch.cat([wd[1:, :, :1], torch.zeros(1, K, 1)], 0)                      # the last chunk gains nothing
        we = torch.cat([wd, extra], 2).clone()
        we[1:, :, 0] = 0.0
        return pool(xe, we.view(nx * K, T + 1), K, F32)
    if fault == "pitch_frames":                       # frames T .. P-1 pooled too, at the weight of the last valid frame
        wd = torch.ones(nx * K, T, dtype=F32) if wr is None else wr
        return pool(xfull, torch.cat([wd, wd[:, -1:].expand(-1, P - T)], 1), K, F32)
    if fault == "swapped_mode":
        return pool(x, resample(w, T, "linear" if mode == "nearest" else "nearest", F32), K, F32)
    if fault == "next_speaker":                       # speaker k pooled with the weights of speaker k + 1
        return pool(x, wr.view(nx, K, T).roll(-1, 1).reshape(nx * K, T), K, F32)
    if fault == "one_pass":                           # moments about one cheap shift per chunk, variance by subtraction
        xk, wd, v1, v2 = _moments(x, wr, K, F32)
        shift = xk[:, :1, :].mean(2, keepdim=True)    # frame 0's mean over the channels
        d = xk - shift
        s1, s2 = (wd[:, :, None] * d).sum(1), (wd[:, :, None] * d * d).sum(1)
        mean = s1 / v1[:, None]
        var = (s2 - s1 * mean) / (v1 - v2 / v1)[:, None]
        return mean + shift[:, 0, :], torch.sqrt(torch.clamp(var, min=0.0))
    raise ValueError(fault)


# --------------------------------------------------------------------------- cases
CIN, NPAD, CHANNELS = 512, 256, 200        # GEMM depth, padded columns, pooled (= stored) columns: 200 = 3 * 64 + 8
JUNK_SHIFT = 10                            # rows T .. P-1 of a chunk carry features 2^10 times the family's: a leak shows

# (pitch P, frames T, chunks)
GEOMETRIES = [(128, 128, 3), (128, 2, 3), (129, 129, 9), (129, 2, 9), (293, 279, 5), (320, 300, 2), (589, 575, 2)]
FEATURES = ["randn", "offset", "sparse"]
SPEAKERS = [1, 2, 3, 4, 5, 8]              # 5, 8: the stand-alone kernel only (groups of four plus a remainder)
FUSED_MAX_K = 4
FAMILIES = ["dense", "peaky", "stretch", "two_frames", "dominant", "degenerate", "unweighted"]


def geom_id(geom):
    return "P%d-T%d-x%d" % geom


def modes(geom):
    """(mode, Fw) the geometry is run with: the production pitch resamples 293 segmentation frames both ways"""
    P, T, _ = geom
    return [("linear", 293), ("nearest", 293), ("identity", T)] if (P, T) == (293, 279) else [("identity", T)]


def families(geom, mode="identity"):
    """Linear resampling computes its source position in float32 (as torch does): at 293 frames one weight moves by up
    to 3e-5 of its neighbours' difference.  Spread over many weighted frames that stays a few 1e-6 in the measure; on a
    support of two to six frames it IS the result (e32 1e-4 .. 1e-3, beyond E32_CAP), so those families are resampled
    by "nearest" and at Fw = T only."""
    if geom[1] == 2:
        return ["dense", "degenerate", "unweighted"]
    return ["dense", "peaky", "degenerate"] if mode == "linear" else FAMILIES


def q22(v):
    """f32 -> the value its two f16 planes hold (hi = f16(v), lo = f16((v - hi) 2^11)): hi + lo / 2^11, exact in f32"""
    v = v.to(F32)
    hi = v.to(torch.float16)
    lo = ((v - hi.float()) * 2048.0).to(torch.float16)
    q = hi.double() + lo.double() / 2048.0
    assert torch.equal(q.float().double(), q)
    return q.float()


@functools.lru_cache(maxsize=None)
def features(geom, family):
    """The GEMM whose float32 output is known bit for bit.  X (nx * P, CIN): row r is 2^s(r) at column j(r), else 0;
    W (NPAD, CIN) >= 0, exact on the 22-bit planes; bias 0, e0 = +-1 per column, e1 = 0: leaky(2^s W[n][j]) * e0 + 0 =
    +- 2^s W[n][j(r)] without a rounding.  -> dict(X, W, e0, y (nx, P, NPAD) float32 = the layer's exact output)"""
    P, T, nx = geom
    g = torch.Generator().manual_seed(1000 * P + 10 * T + FEATURES.index(family))
    r = torch.randn(NPAD, CIN, generator=g)
    if family == "randn":
        v, smax = (r + 0.5).abs(), 1
    elif family == "offset":
        v, smax = 30.0 + 0.01 * r, 0                 # std / mean = 3e-4 in every column: no power of two between the rows
    else:
        v, smax = 3.0 * torch.relu(r), 1
    W = q22(v)
    rows = nx * P
    j = torch.randint(0, CIN, (rows,), generator=g)
    s = torch.randint(-smax, smax + 1, (rows,), generator=g)
    s[(torch.arange(rows) % P) >= T] = JUNK_SHIFT
    X = torch.zeros(rows, CIN)
    X[torch.arange(rows), j] = torch.exp2(s.float())
    e0 = torch.where(torch.rand(NPAD, generator=g) < 0.5, -1.0, 1.0)
    y64 = W.double().t()[j] * torch.exp2(s.double())[:, None] * e0.double()
    y = y64.float()
    assert torch.equal(y.double(), y64)
    return dict(X=X, W=W, e0=e0, y=y.view(nx, P, NPAD))


def boundaries(b, P, T):
    """local frames 0 < t < T of chunk b at which a 128-row tile of the flattened rows begins"""
    return [t for t in range(1, T) if (b * P + t) % TILE == 0]


def _target_weights(family, geom, K, g):
    """(nx * K, T) weights in the frame domain of the features"""
    P, T, nx = geom
    rows = nx * K
    if family == "dense":
        return torch.rand(rows, T, generator=g) ** 2 + 1e-8
    if family == "peaky":
        return torch.rand(rows, T, generator=g) ** 8 + 1e-8
    w = torch.zeros(nx, K, T)
    for b in range(nx):
        bd = boundaries(b, P, T)
        for k in range(K):
            if family == "stretch":                   # exact zeros around one stretch: whole pieces carry s0 = 0
                lo_hi = [(bd[0] - 3, bd[0] + 3) if bd else (T // 2 - 3, T // 2 + 3),              # across a tile boundary
                         (1, max(3, min(6, (bd[0] if bd else T) - 1))),                           # inside the first piece
                         (T - 2, T),                                                              # the last two frames
                         (bd[0] - 2, bd[1] + 2) if len(bd) > 1 else (0, T)][(k + b) % 4]          # three pieces
                lo, hi = max(0, lo_hi[0]), min(T, lo_hi[1])
                w[b, k, lo:hi] = torch.rand(hi - lo, generator=g) + 0.1
            elif family == "two_frames":              # one frame on either side of a tile boundary
                t = bd[k % len(bd)] if bd else 1 + (k + b) % (T - 1)
                w[b, k, t - 1], w[b, k, t] = 0.3 + 0.1 * k, 0.9 - 0.1 * k
            elif family == "dominant":                # kappa ~ 1e5
                w[b, k] = 1e-8
                w[b, k, (37 * b + 11 * k + 5) % T] = 1.0
            elif family == "degenerate":              # one row with a single frame (a power of two), one with none
                kind = (b % 3) if K == 1 else k
                if kind == 0:
                    w[b, k, (7 * b + 1) % T] = 2.0 ** -(b % 3)
                elif kind > 1:
                    w[b, k] = torch.rand(T, generator=g) ** 2 + 1e-8
            else:
                raise ValueError(family)
    return w.view(rows, T)


def weights(family, geom, K, mode, Fw):
    """source weights (nx * K, Fw), speaker-major per chunk, or None.  Built in the frame domain of the features and
    lifted to Fw frames: nearest — exactly (every target frame owns its source frame while Fw >= T); linear — at the
    scaled positions (a single source frame becomes two target frames: no degenerate row but the empty one)."""
    P, T, nx = geom
    if family == "unweighted":
        return None
    g = torch.Generator().manual_seed(97 * P + 13 * T + 7 * K + FAMILIES.index(family))
    if family in ("dense", "peaky") and Fw != T:
        return _target_weights(family, (P, Fw, nx), K, g)
    wt = _target_weights(family, geom, K, g)
    if Fw == T:
        return wt
    assert Fw > T
    idx = nearest_index(Fw, T) if mode == "nearest" else torch.clamp((torch.arange(T) * Fw) // T, max=Fw - 1)
    w = torch.full((wt.shape[0], Fw), 1e-8 if family == "dominant" else 0.0)
    w[:, idx] = wt
    return w


def cells(geom):
    """(K, mode, Fw, family) of one geometry, every feature family alike"""
    return [(K, mode, Fw, fam) for K in SPEAKERS for mode, Fw in modes(geom) for fam in families(geom, mode)
            if not (fam == "unweighted" and mode != modes(geom)[-1][0])]


def expected_degenerate(family, geom, K, mode, Fw):
    """-> (rows with exactly one non-zero resampled weight, rows with none): the rows the inputs are built to have"""
    P, T, nx = geom
    if family != "degenerate":
        return 0, 0
    kinds = [(b % 3) if K == 1 else k for b in range(nx) for k in range(K)]
    single, none = kinds.count(0), kinds.count(1)
    if mode == "linear" and Fw != T:
        single = 0                                   # two target frames share the one source frame
    return single, none


def cell_ref(geom, feat, K, mode, Fw, family):
    """-> (w source weights or None, Ref, e32) of one cell"""
    P, T, nx = geom
    x = features(geom, feat)["y"][:, :T, :CHANNELS]
    w = weights(family, geom, K, mode, Fw)
    ref = Ref(x, None if w is None else resample(w, T, mode, F64), K)
    return w, ref, ref.e32(x, None if w is None else resample(w, T, mode, F32), K)


# --------------------------------------------------------------------------- the random-operand case
RANDOM_GEOM, RANDOM_K, RANDOM_MODE, RANDOM_FW = (293, 279, 5), 3, "linear", 293


@functools.lru_cache(maxsize=None)
def random_case():
    """tdnn5-like operands (as test_gpu_kernels.py::test_gemm_pre): the real k-loop feeds the epilogue.  The reference is
    float64 on the 22-bit operands; den of the measure is taken over |X| |W| (what the contraction summed)."""
    P, T, nx = RANDOM_GEOM
    g = torch.Generator().manual_seed(512)
    rows = nx * P
    X = torch.randn(rows, CIN, generator=g) * 1.5
    W = torch.zeros(NPAD, CIN)
    W[:CHANNELS] = torch.randn(CHANNELS, CIN, generator=g) / math.sqrt(CIN)
    bias = torch.zeros(NPAD)
    bias[:CHANNELS] = torch.randn(CHANNELS, generator=g) * 0.2
    e0, e1 = torch.rand(NPAD, generator=g) + 0.5, torch.randn(NPAD, generator=g) * 0.1
    w = torch.rand(nx * RANDOM_K, RANDOM_FW, generator=g) ** 2 + 1e-8
    Xq, Wq = q22(X).double(), q22(W).double()
    leaky = lambda v: torch.where(v > 0, v, 0.01 * v)
    y = (leaky(Xq @ Wq.t() + bias.double()) * e0.double() + e1.double()).view(nx, P, NPAD)
    mag = ((Xq.abs() @ Wq.abs().t() + bias.abs().double()) * e0.abs().double() + e1.abs().double()).view(nx, P, NPAD)
    ref = Ref(y[:, :T, :CHANNELS], resample(w, T, RANDOM_MODE, F64), RANDOM_K, feature_den=mag[:, :T, :CHANNELS])
    y32 = (leaky(q22(X) @ q22(W).t() + bias) * e0 + e1).view(nx, P, NPAD)
    e32 = max(ref.errors(*pool(y32[:, :T, :CHANNELS], resample(w, T, RANDOM_MODE, F32), RANDOM_K, F32)))
    return dict(X=X, W=W, bias=bias, e0=e0, e1=e1, w=w, ref=ref, e32=e32)
