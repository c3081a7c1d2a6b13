"""Plain CPU model of the d = 64 fp16 / bf16 attention kernels' arithmetic (csrc/attn.hip, csrc/attn_bwd.hip), the references and the per-row metric the
per-row attention tests share, and their input families.  Plain torch on the CPU; one head at a time: q [N, 64], k, v [Nk, 64], float32 tensors whose values
are already representable in T.

The model is a TEST TOOL: it is never compared with a kernel bit for bit (summation order and the hardware exp2 differ).  It exists so that the inputs of
tests/test_attn_paths_gpu.py can be shown, without a GPU, to separate a right kernel from a wrong one (tests/test_attn_model_cpu.py).

Forward, as attn_fwd_kernel / attn_fwd_dma_kernel: c = scale * log2(e); the fp32 chain of q . k starts at -m_ref and c multiplies it inside the exponent
(fp32_scale, what the kernels do today), or q' = round_T(c q) is contracted (what they did; two_term: + round_T(c q - q'), both into the same chain, the cure
that was measured too slow) and the chain holds exponents; 64-key tiles; per 32-query wave the reference maximum m_ref moves in the first tile (to the tile maximum) and whenever
ANY lane's tile maximum exceeds it by THR = 6 — then by a per-lane delta (the lane's tile maximum where that exceeds THR, else 0), with o and l multiplied by
alpha = 2^-delta; p = round_T(2^s) multiplies V and is what the row sum adds up; O = round_T(o / l), lse2 = m_ref + log2(l).
Mutants: "no_o_rescale" / "no_l_rescale" leave the o / l multiplication out (alpha = 1).

References:
    truth_*        float64 softmax attention of the T-rounded inputs (backward: float64 autograd);
    documented_*   float64 evaluation of the kernels' documented arithmetic, softmax over 2^(round_T(c q) . k): what the kernels compute apart from rounding
                   and summation order — differs from the truth by the rounding of q' alone;
    plain_*        the plain same-dtype form in fp32: S = (q k^T) scale, e = round_T(exp(S - rowmax)), O = round_T((e v) / sum e); backward P normalised,
                   dV = round_T(round_T(P)^T dO), dP = dO v^T, D = sum_d dO O, dS = round_T(P o (dP - D)), dQ = round_T(scale dS k), dK = round_T(scale dS^T q).
                   Its error against the truth is E_T, the noise floor every bar is a multiple of.
Metric: row_err = max over rows of max_d |x - truth| / max_d |truth| (a row: the 64 channels of one query, or of one key for dK / dV); the gradients are
also held to the same 2 E_T in head_err, which divides by the largest row maximum of the (image, head) (see there: row_err alone is vacuous for dQ / dK at
spread >= 4).
lse bar (base 2, derived): log2(1 + u) + 2^-17 max_{q,k} sum_d |c q_d k_d|, u = 2^-11 (fp16), 2^-8 (bf16), 2^-24 (fp32): every probability rounded by
(1 +- u), plus 64 fp32 accumulation steps doubled for the -m_ref start and the final log."""
import math

import torch

LOG2E = 1.4426950408889634
THR = 6.0
SCALE = 0.125
U = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8, torch.float32: 2.0 ** -24}
MUTANTS = ("no_o_rescale", "no_l_rescale")


def rnd(x, dtype):
    return x.to(dtype).float()


def _c(scale):
    return (torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)).item()       # the launcher's fp32 product


def scaled_q(q, scale, dtype, two_term):
    """(hi, lo): round_T(c q) and, with two_term, round_T(c q - hi) (the difference is exact in fp32), else None"""
    cq = q.float() * _c(scale)
    hi = rnd(cq, dtype)
    return hi, (rnd(cq - hi, dtype) if two_term else None)


def kernel_fwd(q, k, v, scale, dtype, two_term=False, fp32_scale=False, mutant=None):
    """fp32_scale: the unscaled q is contracted and c multiplies the fp32 accumulator inside the exponent (m_ref, THR and delta in score units) — what the
    kernels do; otherwise q' is single-rounded or two-term.  -> (O [N, 64] float32 holding T values, lse2 [N] float32, moves [waves]: how often each wave moved its reference after the first tile)"""
    assert mutant is None or mutant in MUTANTS, mutant
    N, Nk = q.shape[0], k.shape[0]
    c = _c(scale)
    hi, lo = (q.float(), None) if fp32_scale else scaled_q(q, scale, dtype, two_term)
    e, thr = (c, THR / c) if fp32_scale else (1.0, THR)            # the accumulator times e is the exponent
    k, v = k.float(), v.float()
    out = torch.empty(N, 64)
    lse = torch.empty(N)
    moves = []
    for w0 in range(0, N, 32):
        qh = hi[w0:w0 + 32]
        n = qh.shape[0]
        m_ref = torch.zeros(n)
        o = torch.zeros(n, 64)
        l = torch.zeros(n)
        first, moved = True, 0
        for t0 in range(0, Nk, 64):
            kt, vt = k[t0:t0 + 64], v[t0:t0 + 64]                    # the keys past the end are masked in the kernel: p = 0, left out here
            s = qh @ kt.T
            if lo is not None:
                s = s + lo[w0:w0 + 32] @ kt.T
            s = s - m_ref[:, None]
            mx = s.max(dim=1).values
            if first or bool((mx > thr).any()):
                delta = mx if first else torch.where(mx > thr, mx, torch.zeros_like(mx))
                alpha = torch.ones_like(delta) if first else torch.exp2(-delta * e)
                m_ref = m_ref + delta
                s = s - delta[:, None]
                if mutant != "no_o_rescale":
                    o = o * alpha[:, None]
                if mutant != "no_l_rescale":
                    l = l * alpha
                moved += 0 if first else 1
                first = False
            p = rnd(torch.exp2(s * e), dtype)
            o = o + p @ vt
            l = l + p.sum(dim=1)
        out[w0:w0 + 32] = rnd(o * (1.0 / l)[:, None], dtype)
        lse[w0:w0 + 32] = m_ref * e + torch.log2(l)
        moves.append(moved)
    return out, lse, moves


def kernel_bwd(q, k, v, do, o, lse2, scale, dtype, fp32_scale=False):
    """attn_bwd_dkdv / attn_bwd_dq: P = 2^(s - lse2) in fp32 from the forward's lse2 and O (D = sum_d dO O in fp32), P and dS rounded to T in front of the
    products that consume them, the outputs rounded to T after the multiplication by scale.  s = c (q k^T) with c applied in fp32 (fp32_scale: what the kernels
    do) or round_T(c q) k^T (the single-rounded form they had beside the single-rounded forward).  -> dq, dk, dv (float32 holding T values)"""
    q, k, v, do = q.float(), k.float(), v.float(), do.float()
    s = (q @ k.T) * _c(scale) if fp32_scale else scaled_q(q, scale, dtype, False)[0] @ k.T
    p = torch.exp2(s - lse2.float()[:, None])
    d = (do * o.float()).sum(dim=1)
    ds = rnd(p * (do @ v.T - d[:, None]), dtype)
    return rnd(ds @ k * scale, dtype), rnd(ds.T @ q * scale, dtype), rnd(rnd(p, dtype).T @ do, dtype)


def truth_fwd(q, k, v, scale):
    """float64 -> (O, lse2)"""
    s = (q.double() @ k.double().T) * scale
    return torch.softmax(s, dim=1) @ v.double(), torch.logsumexp(s, dim=1) / math.log(2.0)


def truth_bwd(q, k, v, do, scale):
    qd, kd, vd = (t.double().requires_grad_(True) for t in (q, k, v))
    (torch.softmax((qd @ kd.T) * scale, dim=1) @ vd).backward(do.double())
    return qd.grad, kd.grad, vd.grad


def documented_fwd(q, k, v, scale, dtype):
    """float64 softmax over 2^(round_T(c q) . k) -> (O, lse2)"""
    s2 = scaled_q(q, scale, dtype, False)[0].double() @ k.double().T
    return torch.softmax(s2 * math.log(2.0), dim=1) @ v.double(), torch.logsumexp(s2 * math.log(2.0), dim=1) / math.log(2.0)


def documented_bwd(q, k, v, do, scale, dtype):
    """the header of attn_bwd.hip in float64: P from round_T(c q), dQ = scale dS K, dK = scale dS^T Q with the unscaled q"""
    q, k, v, do = q.double(), k.double(), v.double(), do.double()
    s2 = scaled_q(q.float(), scale, dtype, False)[0].double() @ k.T
    p = torch.softmax(s2 * math.log(2.0), dim=1)
    dp = do @ v.T
    ds = p * (dp - (p * dp).sum(dim=1, keepdim=True))
    return scale * ds @ k, scale * ds.T @ q, p.T @ do


def plain_fwd(q, k, v, scale, dtype):
    s = (q.float() @ k.float().T) * scale
    e = rnd(torch.exp(s - s.max(dim=1, keepdim=True).values), dtype)
    return rnd((e @ v.float()) / e.sum(dim=1, keepdim=True), dtype)


def plain_bwd(q, k, v, do, scale, dtype):
    q, k, v, do = q.float(), k.float(), v.float(), do.float()
    s = (q @ k.T) * scale
    e = torch.exp(s - s.max(dim=1, keepdim=True).values)
    p = e / e.sum(dim=1, keepdim=True)
    d = (do * plain_fwd(q, k, v, scale, dtype)).sum(dim=1, keepdim=True)
    ds = rnd(p * (do @ v.T - d), dtype)
    return rnd(scale * ds @ k, dtype), rnd(scale * ds.T @ q, dtype), rnd(rnd(p, dtype).T @ do, dtype)


def row_err(x, truth):
    """max over rows (all leading dimensions) of max_d |x - truth| / max_d |truth|"""
    x, truth = x.detach().double().cpu(), truth.detach().double().cpu()
    assert x.shape == truth.shape, (x.shape, truth.shape)
    e = (x - truth).abs().reshape(-1, truth.shape[-1]).max(dim=1).values
    m = truth.abs().reshape(-1, truth.shape[-1]).max(dim=1).values
    assert bool((m > 0).all()), "a reference row is all zero"
    return (e / m).max().item()


def head_err(x, truth):
    """x, truth [heads, rows, 64]: max over rows of max_d |x - truth| / (largest max_d |truth| over the rows of the same (image, head)).  The gradients' second
    metric: row_err divides by a row's own maximum, and the float64 gradient of a near-one-hot row is itself about 0, so at a logit spread >= 4 row_err of the
    plain form (E_T) reaches 0.03 ... 2e6 for dQ and dK and a bar built on it checks nothing; this normaliser stays at the size of the head's gradient."""
    x, truth = x.detach().double().cpu(), truth.detach().double().cpu()
    assert x.shape == truth.shape and x.dim() == 3, (x.shape, truth.shape)
    m = truth.abs().amax(dim=(1, 2), keepdim=True).squeeze(2)
    assert bool((m > 0).all()), "a reference head is all zero"
    return ((x - truth).abs().amax(dim=2) / m).max().item()


def lse_bar(q, k, scale, dtype):
    return math.log2(1.0 + U[dtype]) + 2.0 ** -17 * (scale * LOG2E * (q.double().abs() @ k.double().abs().T)).max().item()


# ---- input families (one head; every tensor rounded to T) -------------------------------------------------------------------------------------------------
SPREADS = (1, 4, 8, 16)
CREEP_STEPS = (3.0, 5.9, 6.1)


def _g(seed):
    return torch.Generator().manual_seed(seed)


def late_key(seed, dtype, Nk=320, keys=(200, 270), first3=9.0, lead40=8.0, second3=12.0):
    """N = 128 (four waves).  Base randn; keys[0] scores about +9 (exponent domain) for query 3 and +8 for query 40 (another wave), keys[1] +12 for query 3 and
    +10 for query 70.  The first tile leaves every reference at about 3 - 4, so with these values (the defaults) the 9 and the 8 are leads UNDER the threshold
    of 6 and only keys[1] moves a reference: waves 0 and 2 in the same tile by different deltas, once each, their other 31 lanes passing through the taken
    branch with delta = 0, the earlier keys keeping 10 - 40 % of the row's mass (a wrong alpha is a gross error); waves 1 and 3 never move.
    first3 = 14, lead40 = 13, second3 = 22 (late_key_two_waves): waves 0 and 1 move at keys[0] as well, and wave 0 a second time at keys[1]."""
    g = _g(seed)
    q, k, v = torch.randn(128, 64, generator=g), torch.randn(Nk, 64, generator=g), torch.randn(Nk, 64, generator=g)
    aim = lambda i, bits: q[i] * (bits / LOG2E) * 8.0 / q[i].square().sum()
    k[keys[0]] = aim(3, first3) + aim(40, lead40)
    k[keys[1]] = aim(3, second3) + aim(70, 10.0)
    return rnd(q, dtype), rnd(k, dtype), rnd(v, dtype)


def creep(seed, dtype, step):
    """N = 64, Nk = 512: the scores of tile j sit at j * step (exponent domain): step 3.0 lets the reference lag (probabilities up to 2^6), 5.9 / 6.1 are the two
    sides of the threshold"""
    g = _g(seed)
    c = SCALE * LOG2E
    q, k, v = 0.3 * torch.randn(64, 64, generator=g), 0.3 * torch.randn(512, 64, generator=g), torch.randn(512, 64, generator=g)
    q[:, 0] = 4.0
    k[:, 0] = (torch.arange(512) // 64).float() * step / (4.0 * c) + 0.01 * torch.randn(512, generator=g)
    return rnd(q, dtype), rnd(k, dtype), rnd(v, dtype)


def negative_first_tile(seed, dtype, depth=6.0):
    """N = 96, Nk = 200: every score of tile 0 is strongly negative (the first reference is about -6.5 in the exponent domain; depth 30: about -160, where
    2^-reference is not finite in fp32), the real mass arrives in tile 1"""
    g = _g(seed)
    q, k, v = 0.3 * torch.randn(96, 64, generator=g), 0.3 * torch.randn(200, 64, generator=g), torch.randn(200, 64, generator=g)
    q[:, 0] = depth
    k[:64, 0] = -depth
    k[64:, 0] = 0.2 * 6.0 / depth
    return rnd(q, dtype), rnd(k, dtype), rnd(v, dtype)


def spread(seed, dtype, sigma, N=128, Nk=448):
    """q, k ~ N(0, sigma) (variance sigma: the logits q . k / 8 have standard deviation sigma nats), v ~ N(0, 1)"""
    g = _g(seed)
    q, k, v = torch.randn(N, 64, generator=g), torch.randn(Nk, 64, generator=g), torch.randn(Nk, 64, generator=g)
    return rnd(q * math.sqrt(sigma), dtype), rnd(k * math.sqrt(sigma), dtype), rnd(v, dtype)


RESCALE_FAMILIES = {
    "late_key": lambda seed, dtype: late_key(seed, dtype),
    "late_key_two_waves": lambda seed, dtype: late_key(seed, dtype, first3=14.0, lead40=13.0, second3=22.0),
    "late_key_partial_tile": lambda seed, dtype: late_key(seed, dtype, Nk=300, keys=(200, 290)),
    "creep_3.0": lambda seed, dtype: creep(seed, dtype, 3.0),
    "creep_5.9": lambda seed, dtype: creep(seed, dtype, 5.9),
    "creep_6.1": lambda seed, dtype: creep(seed, dtype, 6.1),
    "negative_first_tile": negative_first_tile,
    "negative_first_tile_deep": lambda seed, dtype: negative_first_tile(seed, dtype, depth=30.0),
}


# ---- the calls the GPU tests make: B images x H heads, every (image, head) its own instance of the family ------------------------------------------------
B, H = 2, 2


def heads_of(family, dtype, seed0=0):
    """[(q, k, v)] for (image, head) = (0, 0), (0, 1), (1, 0), (1, 1): seeds seed0 .. seed0 + 3"""
    return [family(seed0 + i, dtype) for i in range(B * H)]


def pack(mats):
    """B * H matrices [n, 64] (image-major) -> [B, n, H * 64]"""
    return torch.stack([torch.cat(mats[b * H:(b + 1) * H], dim=1) for b in range(B)])


def unpack(t):
    """[B, n, H * 64] -> [B * H, n, 64] (image-major, as heads_of)"""
    t = t.detach().float().cpu()
    return t.reshape(B, t.shape[1], H, 64).permute(0, 2, 1, 3).reshape(B * H, t.shape[1], 64)


def forward_cases(dtype):
    """name -> heads (the rescale families and the spread sweep; the joint and fused-view calls are built from these by the GPU tests)"""
    cases = {name: heads_of(fam, dtype) for name, fam in RESCALE_FAMILIES.items()}
    for sigma in SPREADS:
        cases["spread_%d" % sigma] = heads_of(lambda seed, dt, s=sigma: spread(seed, dt, s), dtype)
    return cases


BACKWARD_NAMES = ["%s_spread_%d" % (kind, s) for s in SPREADS for kind in ("self", "cross")] + ["cross_late_key"]


def backward_cases(dtype):
    """name -> (heads, dO heads, self-attention?): the sweep as self-attention (N = Nk = 192: one and a half query blocks, three key tiles) and as cross-attention
    (N = 128, Nk = 448), family 1 as cross-attention"""
    cases = {}
    for sigma in SPREADS:
        cases["self_spread_%d" % sigma] = (heads_of(lambda seed, dt, s=sigma: spread(seed, dt, s, N=192, Nk=192), dtype, seed0=20), True)
        cases["cross_spread_%d" % sigma] = (heads_of(lambda seed, dt, s=sigma: spread(seed, dt, s), dtype, seed0=30), False)
    cases["cross_late_key"] = (heads_of(late_key, dtype, seed0=40), False)
    out = {}
    assert list(cases) == BACKWARD_NAMES
    for name, (heads, self_attn) in cases.items():
        g = _g(1000 + len(out))
        out[name] = (heads, [rnd(torch.randn(q.shape[0], 64, generator=g), dtype) for q, _, _ in heads], self_attn)
    return out


def forward_refs(heads, dtype, scale=SCALE):
    """-> truth O [BH, N, 64], truth lse2 [BH, N], E_T (pooled over the heads), the lse bar of every head"""
    tr = [truth_fwd(q, k, v, scale) for q, k, v in heads]
    o, lse = torch.stack([t[0] for t in tr]), torch.stack([t[1] for t in tr])
    e_t = row_err(torch.stack([plain_fwd(q, k, v, scale, dtype) for q, k, v in heads]), o)
    return o, lse, e_t, torch.tensor([lse_bar(q, k, scale, dtype) for q, k, _ in heads], dtype=torch.float64)


def backward_refs(heads, dos, dtype, scale=SCALE):
    """-> truth (dq, dk, dv) each [BH, n, 64], E_T of each in row_err, E_T of each in head_err"""
    tr = [truth_bwd(q, k, v, do, scale) for (q, k, v), do in zip(heads, dos)]
    pl = [plain_bwd(q, k, v, do, scale, dtype) for (q, k, v), do in zip(heads, dos)]
    truth = [torch.stack([t[i] for t in tr]) for i in range(3)]
    plain = [torch.stack([p[i] for p in pl]) for i in range(3)]
    return truth, [row_err(plain[i], truth[i]) for i in range(3)], [head_err(plain[i], truth[i]) for i in range(3)]
