"""Float64 restatement of the bidirectional LSTM recurrence (hidden 128) and the operands its tests share.

``bilstm_f64`` is a plain loop over the frames — no ``nn.LSTM`` — of what ``dz_k_lstm`` documents
(include/diart_amd.h): ``gx (B,T,1024)`` is the x-projection with the biases already inside, PyTorch column
order ``dir*512 + gate*128 + unit`` (gates i, f, g, o), ``whh (2,512,128)``; the reverse direction walks
t = T-1 .. 0.  Everything is converted to float64 from the float32 values a kernel is given, so the reference
carries no input rounding of its own.

The rest is shared by ``test_lstm_ref_host.py`` (no GPU: is the restatement right, is every regime well
conditioned in float32) and ``test_gpu_lstm_f64.py`` (the kernels): the input regimes, the float32 ``nn.LSTM``
fed with a given gx (``e32``: how far float32 arithmetic alone is from the reference), and the operand forms of
the kernels (unit-major columns, variant 4's pre-scaling, the W_hh planes).

NaN / Inf INPUTS are not a regime: the model flags such rows before the LSTM, and what ``fminf(NaN, 64)`` makes
of one inside the variant-4 cell is deliberately not a contract.
"""
import functools

import torch

H = 128


# --------------------------------------------------------------------------- the reference
def bilstm_f64(gx: torch.Tensor, whh: torch.Tensor, return_pre: bool = False):
    """gx (B,T,1024) float32, whh (2,512,128) float32 -> h (B,T,256) float64 (columns dir*128 + unit).
    ``return_pre``: also the gate pre-activations (B,T,1024), gx's column order."""
    B, T, C = gx.shape
    assert C == 8 * H and tuple(whh.shape) == (2, 4 * H, H), (gx.shape, whh.shape)
    g64, w64 = gx.detach().cpu().double(), whh.detach().cpu().double()
    out = torch.zeros(B, T, 2 * H, dtype=torch.float64)
    pre_all = torch.zeros(B, T, 8 * H, dtype=torch.float64) if return_pre else None
    for d in range(2):
        h = torch.zeros(B, H, dtype=torch.float64)
        c = torch.zeros(B, H, dtype=torch.float64)
        wt = w64[d].t()
        for t in (range(T) if d == 0 else range(T - 1, -1, -1)):
            pre = g64[:, t, d * 4 * H:(d + 1) * 4 * H] + h @ wt
            i, f = torch.sigmoid(pre[:, :H]), torch.sigmoid(pre[:, H:2 * H])
            g, o = torch.tanh(pre[:, 2 * H:3 * H]), torch.sigmoid(pre[:, 3 * H:])
            c = f * c + i * g
            h = o * torch.tanh(c)
            out[:, t, d * H:(d + 1) * H] = h
            if return_pre:
                pre_all[:, t, d * 4 * H:(d + 1) * 4 * H] = pre
    return (out, pre_all) if return_pre else out


def lstm_on_gx(gx: torch.Tensor, whh: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
    """``torch.nn.LSTM`` (CPU, ``dtype``) run on a GIVEN x-projection: input size 1024, W_ih = the identity
    halves, no bias — ``x W_ih^T`` is then gx exactly (sums of one value and exact zeros)."""
    B, T, _ = gx.shape
    lstm = torch.nn.LSTM(8 * H, H, 1, bidirectional=True, batch_first=True).to(dtype)
    eye = torch.eye(4 * H, dtype=dtype)
    zero = torch.zeros(4 * H, 4 * H, dtype=dtype)
    with torch.no_grad():
        lstm.weight_ih_l0.copy_(torch.cat([eye, zero], 1))
        lstm.weight_ih_l0_reverse.copy_(torch.cat([zero, eye], 1))
        lstm.weight_hh_l0.copy_(whh[0].to(dtype))
        lstm.weight_hh_l0_reverse.copy_(whh[1].to(dtype))
        for n in ("bias_ih_l0", "bias_hh_l0", "bias_ih_l0_reverse", "bias_hh_l0_reverse"):
            getattr(lstm, n).zero_()
        out, _ = lstm(gx.to(dtype))
    return out


def e32_of(gx: torch.Tensor, whh: torch.Tensor, ref: torch.Tensor) -> float:
    """max |float32 nn.LSTM on the CPU - the float64 reference| on this case"""
    return (lstm_on_gx(gx, whh).double() - ref).abs().max().item()


# --------------------------------------------------------------------------- the regimes
REGIMES = ("benign", "saturated8", "saturated32", "overflow", "integrator", "tiny", "zero")
E32_CAP = 1e-5          # a regime in which float32 arithmetic itself drifts further cannot tell a right kernel from a wrong one
WHH_BOUND = 0.25        # U(+-0.25): above, the recurrence stops being contractive (U(+-1) with a forget bias: chaotic)

# sigma of the integrator's random-walking g: with N(0,1) float32 nn.LSTM itself drifts 1.1e-5 at (64, 293) (the rounding of a
# c that walks to +-30 and back to where tanh is steep) — over the cap, so the scale is shrunk, not the cap raised
INTEGRATOR_WALK = 0.6
OVERFLOW_MAGNITUDES = (100.0, 200.0, 1e4, 1e30)
# gate patterns of the forced units, (i, f, g, o) signs, 0 = left alone: every gate alone in each sign, then all four
OVERFLOW_PATTERNS = tuple(tuple(s if k == gate else 0 for k in range(4)) for gate in range(4) for s in (1, -1)) + (
    (1, 1, 1, 1), (-1, -1, -1, -1), (1, 1, -1, 1), (1, -1, 1, -1))


def force_overflow(gx: torch.Tensor, chain: int, shift: int = 0) -> None:
    """In place: chain ``chain`` of gx (PyTorch column order) gets, for the whole sequence and in both
    directions, one hidden unit per (pattern, magnitude) of the tables above forced to +-magnitude on the
    pattern's gates — 48 of the 128 units, placed by ``shift`` so that different chains hit different lanes."""
    k = 0
    for pat in OVERFLOW_PATTERNS:
        for mag in OVERFLOW_MAGNITUDES:
            unit = (37 * k + 11 + shift) % H          # 37 is odd: the 48 slots are distinct units
            for gate, sign in enumerate(pat):
                if sign:
                    for d in range(2):
                        gx[chain, :, d * 4 * H + gate * H + unit] = sign * mag
            k += 1


def overflow_chains(B: int):
    return sorted({0, 5 % B, B - 1, 16 % B})


def make_case(regime: str, B: int, T: int):
    """-> (gx (B,T,1024) float32 in PyTorch column order, whh (2,512,128) float32), seeded by (regime, B, T)"""
    g = torch.Generator().manual_seed(1000 * REGIMES.index(regime) + 100 * B + T)
    whh = (torch.rand(2, 4 * H, H, generator=g) * 2 - 1) * WHH_BOUND
    n = torch.randn(B, T, 8 * H, generator=g)
    if regime == "benign":
        gx = n * 0.8
    elif regime == "saturated8":
        gx = n * 8.0
    elif regime == "saturated32":
        gx = n * 32.0
    elif regime == "tiny":
        gx = n * 1e-3
    elif regime == "zero":
        gx, whh = torch.zeros_like(n), torch.zeros_like(whh)
    elif regime == "overflow":
        gx = n * 0.8
        for chain in overflow_chains(B):
            force_overflow(gx, chain, shift=3 * chain)
    elif regime == "integrator":
        # W_hh = 0; i, f wide open: c_t = c_{t-1} + tanh(g).  Units 0..63: g = +-20 with a fixed sign per unit, c = +-t;
        # units 64..127: g ~ N(0, WALK), c random-walks (through +-22, where variant 4's exp2 argument crosses its clamp)
        whh = torch.zeros_like(whh)
        v = n.view(B, T, 2, 4, H).clone()
        v[:, :, :, 2, H // 2:] *= INTEGRATOR_WALK
        v[:, :, :, 0, :] = 20.0
        v[:, :, :, 1, :] = 20.0
        sign = torch.where(torch.arange(H // 2) % 3 == 0, -1.0, 1.0)
        v[:, :, :, 2, :H // 2] = 20.0 * sign
        gx = v.view(B, T, 8 * H)
    else:
        raise ValueError(regime)
    return gx.float().contiguous(), whh.float().contiguous()


@functools.lru_cache(maxsize=2)
def case(regime: str, B: int, T: int):
    """-> (gx, whh, float64 reference, e32) of ``make_case`` (the last two cases are kept: every kernel of a case
    runs before the next case starts)"""
    gx, whh = make_case(regime, B, T)
    ref = bilstm_f64(gx, whh)
    return gx, whh, ref, e32_of(gx, whh, ref)


# --------------------------------------------------------------------------- what the kernels are given
KERNELS = ("valu", "mfma0", "mfma0_um", "mfma1", "mfma1_um", "mfma2", "mfma2_um", "mfma3_um", "mfma4_um")


def unit_major(gx: torch.Tensor) -> torch.Tensor:
    """columns dir*512 + gate*128 + unit -> dir*512 + unit*4 + gate (what the projection GEMM of the model writes)"""
    B, T, _ = gx.shape
    return gx.view(B, T, 2, 4, H).transpose(3, 4).reshape(B, T, 8 * H).contiguous()


def prescale_um(gx_um: torch.Tensor) -> torch.Tensor:
    """unit-major gx times the gates' activation scales, rounded to float32: what variant 4 is given (that rounding is
    part of the kernel's error, the reference runs on the unscaled values)"""
    from diart_amd.weights import LSTM_GATE_SCALE
    B, T, _ = gx_um.shape
    sc = torch.tensor(LSTM_GATE_SCALE, dtype=torch.float64)
    return (gx_um.double().view(B, T, 2 * H, 4) * sc).float().view(B, T, 8 * H).contiguous()


def kernel_operands(kernel: str, gx: torch.Tensor, whh: torch.Tensor):
    """-> (gx as the kernel reads it, its W_hh operand, unit_major flag, variant; -1 = the f32 vector kernel)"""
    from diart_amd.weights import lstm_whh_planes
    if kernel == "valu":
        return gx.contiguous(), whh.contiguous(), 0, -1
    um, variant = kernel.endswith("_um"), int(kernel[4])
    if um:
        gx = unit_major(gx)
    if variant >= 4:
        gx = prescale_um(gx)
    return gx.contiguous(), lstm_whh_planes(whh, variant), int(um), variant


# --------------------------------------------------------------------------- the stack through the model
STACK_FACTOR, STACK_FORGET_BIAS, STACK_LAYERS = 8.0, 3.0, (0,)


def saturating_segmentation_state(factor: float = STACK_FACTOR, forget_bias: float = STACK_FORGET_BIAS, layers=STACK_LAYERS):
    """``synth_segmentation_state()`` with ``lstm.weight_ih_l{layer}*`` times ``factor`` and ``forget_bias`` added to the
    forget quarter of ``lstm.bias_ih_l{layer}*`` for every layer in ``layers``.  W_hh is untouched (its bound
    1.6 / sqrt(128) keeps a layer contractive).  Only layer 0 by default: it saturates (19 % of its gate pre-activations
    beyond |8|) and hands layers 1..3 — the x-projection epilogue and the recurrence's own planes — an h that sits at
    +-1 and 0, while the float32 stack stays 2.5e-6 from float64.  With all four layers modified the float32 stack
    drifts 1e-4 before the regime is reached (test_lstm_ref_host.py asserts both facts)."""
    from diart_amd.synth import synth_segmentation_state
    sd = {k: v.clone() for k, v in synth_segmentation_state().items()}
    for k in sd:
        for stem, what in (("lstm.weight_ih_l", "w"), ("lstm.bias_ih_l", "b")):
            if k.startswith(stem) and int(k[len(stem)]) in layers:
                if what == "w":
                    sd[k] = sd[k] * factor
                else:
                    sd[k][H:2 * H] += forget_bias
    return sd


def stack_windows(n: int = 16):
    """``n`` windows of 5 s of the synthetic streams, (n, 80000) float32"""
    from diart_amd.synth import synth_streams
    return torch.from_numpy(synth_streams(n, 5.0, seed0=777))[:, :80000].contiguous()


def oracle_segmentation(sd, audio: torch.Tensor) -> torch.Tensor:
    """``PyanNetRef`` (float32, as the project's gates use it) with ``sd`` on ``audio (B, S)`` -> (B, F, K)"""
    from oracle.models_ref import PyanNetRef
    m = PyanNetRef().eval()
    m.load_state_dict(sd)
    with torch.no_grad():
        return m(audio[:, None, :])


def stack_reference_f64(sd, audio: torch.Tensor, return_frac: bool = False):
    """The segmentation network with its four LSTM layers restated in float64 by ``bilstm_f64``.

    The oracle module does not run in float64 as it stands: its SincNet in float64 differs from its float32 self by
    1.5e-4 at the SincNet output (5.7e-5 at the network output with the unmodified synthetic state) — the front end's
    conditioning, not the recurrence's.  So the SincNet stays the oracle's float32 module (its output is the float32
    input the LSTM stack is given), the stack is ``x W_ih^T + b_ih + b_hh -> bilstm_f64`` per layer, and the head is
    the oracle's formulas in float64.  ``return_frac``: also the fraction of layer-0 gate pre-activations beyond |8|."""
    import torch.nn.functional as F
    from oracle.models_ref import PyanNetRef
    m = PyanNetRef().eval()
    m.load_state_dict(sd)
    with torch.no_grad():
        x = m.sincnet(audio[:, None, :]).transpose(1, 2).double()                    # (B, F, 60)
    d = lambda k: sd[k].detach().double()
    frac = None
    for layer in range(4):
        gx = torch.cat([x @ d(f"lstm.weight_ih_l{layer}{s}").t() + d(f"lstm.bias_ih_l{layer}{s}") + d(f"lstm.bias_hh_l{layer}{s}")
                        for s in ("", "_reverse")], -1)
        whh = torch.stack([d(f"lstm.weight_hh_l{layer}"), d(f"lstm.weight_hh_l{layer}_reverse")])
        if layer == 0 and return_frac:
            x, pre = bilstm_f64(gx, whh, return_pre=True)
            frac = (pre.abs() > 8).double().mean().item()
        else:
            x = bilstm_f64(gx, whh)
    for i in range(2):
        x = F.leaky_relu(x @ d(f"linear.{i}.weight").t() + d(f"linear.{i}.bias"))
    out = torch.sigmoid(x @ d("classifier.weight").t() + d("classifier.bias"))
    return (out, frac) if return_frac else out
