"""The saturated-gate automaton: weights under which MiniROAD / MiniROADA have ONE right answer in every compute dtype and every pass
(tests/test_gru_automaton_cpu.py, tests/test_gpu_automaton.py).

The method.  Every gate pre-activation is kept at least 32 away from zero, so in fp32 r and z are exactly 0-or-1 (the 0 side is below
2^-46, which no sum with a +-1 sees) and n is exactly +-1.  h' = (1 - z) n + z h is then a SELECTION, h_t lies in {-1, 0, +1}^H (0 only
while a unit has never been written), and the model is a boolean network that a few integer operations compute:

  features    rows of 0/1 bits
  layer1.0    a column selection (one 1 per row, zero bias): Y_j = x_sigma(j) exactly; LayerNorm gamma 1, beta 0.  After LayerNorm + ReLU a
              one-bit is c = (1 - p) / sqrt(p (1 - p) + eps) (about 1; p = the row's share of ones) and a zero-bit is exactly 0
  W_ih        one +128 per row, at column pi(row); b_ih = -64 - 128 a, b_hh = +128 a (a in {-1, 0, 1}, 0 on the n rows): the two biases sum
              to -64, and a path that forgets either of them changes decisions.  gi is 128 c - 64 (about +64) or exactly -64
  W_hh        entries 0 / +-128: sparse rows with an EVEN number of nonzeros (so that gh = 0 happens and the input decides), some rows
              fully dense; the columns cover [0, H) in every gate.  gh is an exact multiple of 128 below 2^18
  b_hn        from {-128, 0, +128}
  2nd layer   the same scheme on the first layer's h_t: gi = 128 h[pi] - 64 in {+64, -64, -192}
  head        f_classification = head_scale * integers of [-8, 8] \\ {0}: every unit of relu(h) moves the logits of its own frame, logits
              are exact multiples of head_scale; some class rows are DUPLICATES of earlier ones (far apart, adjacent, 16 apart), so exact
              two- and three-way ties for the maximum occur and "first maximum wins" is tested
  MiniROADA   anticipation_layer: 4 small integers per row, A_l = relu(relu(h) W_a[l]^T + b_a[l]) stays an integer <= 10

Every pre-activation is an odd multiple of 64 moved by 128 (c - 1): sign(pre) is what the automaton computes.  sigmoidf_ (csrc/common.h)
gives exactly 1 for x > 17.33 (exp(-x) < 2^-25, 1 + e rounds to 1) and at most exp(-32) = 1.3e-14 for x < -32; tanhf_ is exactly +-1 beyond |x| = 9.02
(2 / (1 + exp(2 |x|)) < 2^-25).
128, 64, 8 and +-1 are exact in bf16, fp16 and fp16x2's hi/lo split; what a 16-bit mode does round (c, and gi = 128 c - 64 where the pass
keeps it in 16 bits) moves a pre-activation by at most 256 * 2^-8 = 1, far inside the margin of 32.

Integer-valued matrix products with every partial sum below 2^24 are exact in fp32 in any order, so torch's own BLAS (independent of the
kernels under test) computes the reference, on the CPU or the GPU.  Nothing in this module is a number read off a kernel."""
import math
from dataclasses import dataclass, field

import numpy as np
import torch

AMP = 128.0
PRE_FLOOR = 32.0              # derived 17.33 (exact saturation of sigmoidf_ / tanhf_ in fp32) with margin
LN_EPS = 1e-5
U = 2.0 ** -24                # unit roundoff of fp32 (half an ulp of 1)


@dataclass(frozen=True)
class Case:
    d_rgb: int = 2048
    d_flow: int = 0
    emb: int = 2048
    hid: int = 1024
    n_classes: int = 12
    num_layers: int = 1
    ant_len: int = 0
    seed: int = 0
    nnz: int = 8                  # nonzeros of a sparse W_hh row (even)
    head_scale: float = 1.0       # a power of two; 1/32 keeps the logit spread of the probability cases below 60


def _gru_layer(rng, H, in_dim, nnz):
    w_ih = np.zeros((3 * H, in_dim), np.float32)
    pi = np.concatenate([rng.permutation(in_dim) for _ in range((3 * H + in_dim - 1) // in_dim)])[:3 * H]      # every input column is read
    w_ih[np.arange(3 * H), pi] = AMP
    a = rng.integers(-1, 2, 3 * H)
    a[2 * H:] = 0                                          # b_hn sits behind r: only b_in = -64 keeps the n row an odd multiple of 64
    b_ih = (-64.0 - AMP * a).astype(np.float32)
    b_hh = (AMP * a).astype(np.float32)
    b_hh[2 * H:] = AMP * rng.integers(-1, 2, H)
    w_hh = np.zeros((3 * H, H), np.float32)
    dense = rng.random(3 * H) < 1.0 / 64
    dense[[0, H, 2 * H]] = True                            # at least one dense row per gate: every column of W_hh is used in each gate
    for row in range(3 * H):
        if dense[row]:
            w_hh[row] = AMP * rng.choice([-1.0, 1.0], H)
        else:
            w_hh[row, rng.choice(H, nnz, replace=False)] = AMP * rng.choice([-1.0, 1.0], nnz)
    return w_ih, w_hh, b_ih, b_hh, pi


def build_state_dict(case: Case):
    """(state dict of fp32 CPU tensors with the reference's names, meta): meta holds the index form of the one-entry-per-row matrices
    (sigma, pi per layer) that the automaton reads instead of multiplying by them"""
    assert case.nnz % 2 == 0 and case.emb <= case.d_rgb + case.d_flow
    rng = np.random.default_rng(1000 + case.seed)
    din, E, H, C = case.d_rgb + case.d_flow, case.emb, case.hid, case.n_classes
    sigma = rng.permutation(din)[:E]                        # injective: a balanced feature builder can set every Y_j on its own
    w1 = np.zeros((E, din), np.float32)
    w1[np.arange(E), sigma] = 1.0
    sd = {"layer1.0.weight": w1, "layer1.0.bias": np.zeros(E, np.float32),
          "layer1.1.weight": np.ones(E, np.float32), "layer1.1.bias": np.zeros(E, np.float32)}
    meta = {"sigma": sigma, "pi": []}
    for l in range(case.num_layers):
        w_ih, w_hh, b_ih, b_hh, pi = _gru_layer(rng, H, E if l == 0 else H, case.nnz)
        sd[f"gru.weight_ih_l{l}"], sd[f"gru.weight_hh_l{l}"], sd[f"gru.bias_ih_l{l}"], sd[f"gru.bias_hh_l{l}"] = w_ih, w_hh, b_ih, b_hh
        meta["pi"].append(pi)
    wc = rng.integers(1, 9, (C, H)) * rng.choice([-1, 1], (C, H))
    bc = rng.integers(-3, 4, C)
    # duplicated class rows: whenever one of them is the maximum there is an exact tie.  The pairs sit where an argmax reduction can
    # go wrong in different ways: far apart (0, C-1), neighbours inside one group of four (1, 2), and 16 apart (1, 17), (5, 33) - the
    # heads keep classes c, c + 16, ... (and, in one kernel, c .. c + 3) on one lane and the rest on others.  A bias of about half the
    # logits' spread on the first row of each set makes ties frequent, not constant
    for first, copy in ((0, C - 1), (1, 2), (1, 17), (5, 33)):
        if copy < C and copy != first:
            bc[first] = bc[first] % 4 + 64 * max(1, H // 1024)
            wc[copy], bc[copy] = wc[first], bc[first]
    sd["f_classification.0.weight"] = (case.head_scale * wc).astype(np.float32)
    sd["f_classification.0.bias"] = (case.head_scale * bc).astype(np.float32)
    if case.ant_len:
        L = case.ant_len
        wa = np.zeros((L * H, H), np.float32)
        for row in range(L * H):
            wa[row, rng.choice(H, 4, replace=False)] = rng.choice([-2.0, -1.0, 1.0, 2.0], 4)
        sd["anticipation_layer.0.weight"] = wa
        sd["anticipation_layer.0.bias"] = rng.integers(-1, 3, L * H).astype(np.float32)
    return {k: torch.from_numpy(v) for k, v in sd.items()}, meta


def build_features(case: Case, lens, seed, device="cpu", balanced=False, sigma=None):
    """per clip (rgb [T, d_rgb], flow [T, d_flow] or None): fp32 rows of 0/1 bits, built on `device`.  balanced: exactly half of the emb
    selected columns are ones in every row (p = 1/2, c = 0.99998: the training case's gradient bound needs |pre| >= 64 - 0.003)"""
    g = torch.Generator(device=device)
    g.manual_seed(7000 + seed)
    din, out = case.d_rgb + case.d_flow, []
    for T in lens:
        x = (torch.rand((T, din), device=device, generator=g) < 0.5).to(torch.float32)
        if balanced:
            order = torch.rand((T, case.emb), device=device, generator=g).argsort(dim=1)
            x[:, torch.as_tensor(sigma, device=device)] = (order < case.emb // 2).to(torch.float32)
        out.append((x[:, :case.d_rgb].contiguous() if case.d_rgb else None, x[:, case.d_rgb:].contiguous() if case.d_flow else None))
    return out


def first_argmax(x):
    """index of the FIRST maximal element of every row (spelled out: no reliance on a library's tie rule)"""
    C = x.shape[-1]
    ar = torch.arange(C, device=x.device).expand_as(x)
    return torch.where(x == x.max(dim=-1, keepdim=True).values, ar, C).min(dim=-1).values.to(torch.int32)


@dataclass
class Result:
    lens: list
    offs: list
    h: list                       # per layer int8 [frames, H]: h_t of every frame, clip after clip
    h_last: torch.Tensor          # fp32 [n, H] or [layers, n, H]
    logits: torch.Tensor          # fp64 [frames, C], exact
    argmax: torch.Tensor          # int32 [frames]
    ant_logits: torch.Tensor = None      # fp64 [frames, L, C]
    ant_argmax: torch.Tensor = None
    stats: dict = field(default_factory=dict)

    def clip(self, t, i):
        return t[self.offs[i]:self.offs[i] + self.lens[i]]


def _recur(inp, amp_in, c_one, b_ih, w_hh_t, b_hh, lens_t, offs_t, h0, stats):
    """one GRU layer.  inp int8 [frames, 3H]: the input element each gate row reads (a feature bit / the lower layer's h); its gi is
    amp_in * c_one * inp + b_ih, c_one fp64 [frames] = what LayerNorm makes of a one-bit (None: exactly 1)."""
    n, H = h0.shape
    dev = h0.device
    lens = lens_t.cpu().numpy()
    maxT, total = int(lens.max()), inp.shape[0]
    order = np.argsort(-lens, kind="stable")                  # longest first: the clips alive at step t are the first k_t of this order
    order_t = torch.as_tensor(order, device=dev)
    live = [int((lens > t).sum()) for t in range(maxT)]
    offs_s = offs_t[order_t]
    hs = torch.zeros((total, H), dtype=torch.int8, device=dev)
    h = h0[order_t].clone()
    flips = torch.zeros(maxT, dtype=torch.float64, device=dev)
    min_pre = torch.full((), float("inf"), dtype=torch.float64, device=dev)
    max_gh = torch.zeros((), dtype=torch.float64, device=dev)
    one, minus = torch.ones((), device=dev), -torch.ones((), device=dev)
    for t in range(maxT):
        k = live[t]
        idx = offs_s[:k] + t
        hk = h[:k]
        g = amp_in * inp[idx].to(torch.float64)
        if c_one is not None:
            g = g * c_one[idx, None]
        g = g + b_ih
        gh = (hk @ w_hh_t).to(torch.float64) * AMP + b_hh         # h and W_hh / 128 hold 0 / +-1: exact in fp32 in any order
        pr, pz = g[:, :H] + gh[:, :H], g[:, H:2 * H] + gh[:, H:2 * H]
        pn = g[:, 2 * H:] + (pr > 0) * gh[:, 2 * H:]
        hn = torch.where(pz > 0, hk, torch.where(pn > 0, one, minus))
        min_pre = torch.minimum(min_pre, torch.minimum(torch.minimum(pr.abs().min(), pz.abs().min()), pn.abs().min()))
        max_gh = torch.maximum(max_gh, gh.abs().max())
        flips[t] = (hn != hk).sum() / (k * H)
        h[:k] = hn
        hs[idx] = hn.to(torch.int8)
    stats.setdefault("min_pre", []).append(float(min_pre))
    stats.setdefault("max_gh", []).append(float(max_gh))
    stats.setdefault("flips", []).append(flips.cpu())
    out = torch.empty_like(h)
    out[order_t] = h
    return hs, out


def run(sd, meta, case: Case, feats, h0=None, device=None):
    """the automaton over ragged clips.  feats: build_features' list; h0: None or [n, H] / [layers, n, H] of {-1, 0, 1}"""
    dev = torch.device(device if device is not None else feats[0][0].device if feats[0][0] is not None else feats[0][1].device)
    H, C, L = case.hid, case.n_classes, case.num_layers
    lens = [int((r if r is not None else f).shape[0]) for r, f in feats]
    offs = [0]
    for T in lens[:-1]:
        offs.append(offs[-1] + T)
    lens_t, offs_t = torch.tensor(lens, device=dev), torch.tensor(offs, device=dev)
    n = len(lens)
    sigma = torch.as_tensor(meta["sigma"], device=dev)
    col0 = sigma[torch.as_tensor(meta["pi"][0], device=dev)]
    bits, shares = [], []
    for r, f in feats:
        x = torch.cat([t.to(dev) for t in (r, f) if t is not None], dim=1)
        bits.append(x[:, col0].to(torch.int8))
        shares.append(x[:, sigma].to(torch.float64).mean(dim=1))
        assert bool(((x == 0) | (x == 1)).all())
    inp, p = torch.cat(bits), torch.cat(shares)
    c_one = (1.0 - p) / torch.sqrt(p * (1.0 - p) + LN_EPS)        # nn.LayerNorm in fp64: (1 - mean) / sqrt(biased var + eps)
    stats = {"p_min": float(p.min()), "p_max": float(p.max()), "c_min": float(c_one.min()), "c_max": float(c_one.max())}
    hs_all, h_last = [], []
    for l in range(L):
        g = lambda k: sd[k].to(dev)
        w_hh_t = (g(f"gru.weight_hh_l{l}") / AMP).t().contiguous()
        if h0 is None:
            h_init = torch.zeros((n, H), dtype=torch.float32, device=dev)
        else:
            h_init = (h0 if (L == 1 and h0.dim() == 2) else h0[l]).to(dev, torch.float32)
        if l > 0:
            inp, c_one = hs_all[-1][:, torch.as_tensor(meta["pi"][l], device=dev)], None
        hs, h = _recur(inp, AMP, c_one, g(f"gru.bias_ih_l{l}").to(torch.float64), w_hh_t, g(f"gru.bias_hh_l{l}").to(torch.float64),
                       lens_t, offs_t, h_init, stats)
        hs_all.append(hs)
        h_last.append(h)
    wc, bc = sd["f_classification.0.weight"].to(dev, torch.float64), sd["f_classification.0.bias"].to(dev, torch.float64)
    total = hs_all[-1].shape[0]
    logits = torch.empty((total, C), dtype=torch.float64, device=dev)
    ant = torch.empty((total, case.ant_len, C), dtype=torch.float64, device=dev) if case.ant_len else None
    max_a = 0.0
    for s in range(0, total, 16384):
        hr = hs_all[-1][s:s + 16384].clamp(min=0).to(torch.float64)
        logits[s:s + 16384] = hr @ wc.t() + bc
        if case.ant_len:
            wa, ba = sd["anticipation_layer.0.weight"].to(dev, torch.float64), sd["anticipation_layer.0.bias"].to(dev, torch.float64)
            a = torch.relu(hr @ wa.t() + ba).view(-1, case.ant_len, H)            # rows l H .. l H + H - 1 of the weight are step l
            max_a = max(max_a, float(a.max()))
            ant[s:s + 16384] = a @ wc.t() + bc
    res = Result(lens, offs, hs_all, h_last[0] if L == 1 else torch.stack(h_last), logits, first_argmax(logits))
    if case.ant_len:
        res.ant_logits, res.ant_argmax = ant, first_argmax(ant)
        stats["max_A"] = max_a
    mx = logits.max(dim=1, keepdim=True).values
    stats["tie_frames"] = int(((logits == mx).sum(dim=1) > 1).sum())
    stats["frames"] = total
    stats["max_logit_units"] = float(logits.abs().max()) / case.head_scale
    stats["spread"] = float((mx[:, 0] - logits.min(dim=1).values).max())
    stats["on"] = float((hs_all[0] > 0).to(torch.float64).mean())
    res.stats = stats
    return res


def _exact_in_16bit(t):
    t = t.to(torch.float32)
    return bool((t.to(torch.bfloat16).to(torch.float32) == t).all()) and bool((t.to(torch.float16).to(torch.float32) == t).all())


def conditions(sd, case: Case, res: Result, want_ties=True, max_spread=None):
    """what a case must satisfy FROM THE REFERENCE ALONE before a GPU result is looked at; returns the figures"""
    st = res.stats
    # 1. saturation: every gate pre-activation of every live (clip, frame, unit), with gi from the real fp64 LayerNorm output
    assert min(st["min_pre"]) >= PRE_FLOOR, st["min_pre"]
    # 2. what a 16-bit mode rounds is exactly representable in it (weights, biases that meet 16-bit operands, features and states are
    #    0 / +-1); c and the gi built from it are not: |gi| < 256 rounds by at most 256 * 2^-8 = 1 in bf16, covered by the floor of 32
    for k, v in sd.items():
        assert _exact_in_16bit(v), k
    #    fp16x2 splits layer1.0.weight, W_ih and W_hh into hi = fp16(w * sc), lo = fp16(w * sc - hi) under the power of two sc that
    #    puts the matrix's largest magnitude into [8192, 16384) (csrc/rowwise.hip): hi must be exact and lo zero
    for k in ("layer1.0.weight", "gru.weight_ih_l0", "gru.weight_hh_l0"):
        w = sd[k].to(torch.float64)
        scaled = w * 2.0 ** (14 - math.frexp(float(w.abs().max()))[1])
        assert bool((scaled.to(torch.float16).to(torch.float64) == scaled).all()), k
    assert max(st["max_gh"]) < 2 ** 24 and st.get("max_A", 0.0) <= 256
    assert 0.40 <= st["p_min"] and st["p_max"] <= 0.64, (st["p_min"], st["p_max"])      # c in [0.75, 1.25]: 128 c - 64 in [32, 128 - 32]
    # 3. live dynamics: 10 % .. 40 % of the units change per step once the start has washed out
    for fl in st["flips"]:
        tail = fl[5:]
        if len(tail):
            assert 0.10 <= float(tail.min()) and float(tail.max()) <= 0.40, (float(tail.min()), float(tail.max()))
    # 4. exact logits
    assert st["max_logit_units"] < 2 ** 24
    # 5. ties for the maximum: at least one frame in 50
    if want_ties and st["frames"] >= 50:
        assert st["tie_frames"] * 50 >= st["frames"], (st["tie_frames"], st["frames"])
    if max_spread is not None:
        assert st["spread"] <= max_spread, st["spread"]
    return st


# ---- fp32 emulation of the device functions (csrc/common.h), for the CPU test of the claims above ----------------------------------
def sigmoid_f32(x):
    x = np.asarray(x, np.float32)
    with np.errstate(over="ignore", divide="ignore"):
        return (np.float32(1.0) / (np.float32(1.0) + np.exp(-x).astype(np.float32))).astype(np.float32)


def tanh_f32(x):
    x = np.asarray(x, np.float32)
    with np.errstate(over="ignore", divide="ignore"):
        return (np.float32(2.0) * (np.float32(1.0) / (np.float32(1.0) + np.exp(np.float32(-2.0) * x).astype(np.float32))) - np.float32(1.0)).astype(np.float32)


def gru_step_f32(gi, h, w_hh, b_hh):
    """one step with the kernels' formulas in fp32: r, z = sigmoidf_, n = tanhf_(gi_n + r (gh_n + b_hn)), h' = (1 - z) n + z h"""
    H = h.shape[-1]
    one = np.float32(1.0)
    gh = (h @ w_hh.T).astype(np.float32)
    r = sigmoid_f32(gi[:, :H] + gh[:, :H] + b_hh[:H])
    z = sigmoid_f32(gi[:, H:2 * H] + gh[:, H:2 * H] + b_hh[H:2 * H])
    n = tanh_f32(gi[:, 2 * H:] + r * (gh[:, 2 * H:] + b_hh[2 * H:]))
    return ((one - z) * n + z * h).astype(np.float32)


# ---- derived bounds ------------------------------------------------------------------------------------------------------------------
# __expf(d) is v_exp_f32(d * log2(e)): the constant is rounded (<= 2^-25 relative), the product is rounded (<= 2^-24), so the exponent
# is off by at most 1.5 |d| log2(e) 2^-24 and the result by the factor 2^that = 1 + 1.5 |d| 2^-24; the instruction itself is good to
# 1 ulp <= 2^-23 relative (csrc/common.h).  Hence  rel. error of __expf(d) <= (1.5 |d| + 2) 2^-24.
def exp_rel_bound(d):
    return (1.5 * np.abs(d) + 2.0) * U


# sigmoidf_(x) = rcp(1 + e), e = __expf(-x), s = 1 / (1 + e):  ds/de = -s^2 and s^2 e = s (1 - s), so the error of e moves s by
# s (1 - s) (1.5 |x| + 2) 2^-24 <= (1.5 * 0.2239 + 2 * 0.25) 2^-24 = 0.836 * 2^-24   (|x| s (1 - s) peaks at 0.2239, |x| = 1.5434);
# the rounding of 1 + e is <= 2^-24 relative and rcp's 1 ulp <= 2^-23 relative, of s <= 1: together 3 * 2^-24.  Sum 3.84 -> 4.
SIGMOID_ABS_BOUND = 4.0 * U
# tanhf_(x) = 2 sigmoid(2 x) - 1: 2 x and 2 s are exact, the subtraction rounds a result of magnitude <= 1 by <= 2^-25:
# 2 * 3.84 + 0.5 = 8.18 -> 9.
TANH_ABS_BOUND = 9.0 * U
# what the ABI shows of sigmoidf_ is h_1 = (1 - z) * 1 + z * 0: one more rounding of a number <= 1 (2^-25)
ONE_MINUS_SIGMOID_ABS_BOUND = 4.5 * U
# tanhf_(sigmoidf_(x) * 1 + 0): |tanh'| <= 1 carries the sigmoid's error through, plus tanhf_'s own
TANH_OF_SIGMOID_ABS_BOUND = 13.0 * U


def softmax_bound(logits64):
    """bound on |p - p64| per element for the head's softmax (csrc/head_softmax.hip, csrc/ant_head.hip): e_c = __expf(x_c - max),
    s = sum of the e_c over the C classes (padded with zeros to a multiple of 16) in fp32, p_c = e_c * (1 / s).
      * x_c - max is exact (the logits are exact multiples of head_scale below 2^24 units)
      * e_c carries (1.5 d_c + 2) 2^-24 relative, d_c = |x_c - max|
      * s: the errors of its terms average with weights p_c: sum_c p_c (1.5 d_c + 2) <= 2 + 1.5 (C - 1) / e  (d exp(-d) <= 1 / e,
        p_c <= exp(-d_c), the maximum itself has d = 0) <= 2 + 0.56 C; the additions, in any order, add at most (C_pad - 1) 2^-24
        <= (C + 14) 2^-24
      * 1 / s to 1 ulp (2 * 2^-24) and the product's rounding (2^-24)
    relative error of p_c <= (1.5 d_c + 1.56 C + 21) 2^-24; second-order terms are below 1e-3 of that and ride in the rounding up of
    1.56 to 1.6 and 21 to 22.  The form is p (a |x - max| + b C + c) 2^-24 with a = 1.5, b = 1.6, c = 22."""
    x = logits64
    d = x.max(dim=-1, keepdim=True).values - x
    p = torch.softmax(x, dim=-1)
    return p, p * (1.5 * d + 1.6 * x.shape[-1] + 22.0) * U


def trunk_grad_factor(sd, case: Case, dlogits, rows):
    """F with |every trunk gradient element| <= sigmoid(-64) * F for the balanced training case (p = 1/2: every pre-activation is at
    least 63.99 from zero; a 16-bit c rounds to exactly 1).  Saturated gates pass no gradient: 1 - n^2 is exactly 0 (n = +-1), z (1 - z)
    and r (1 - r) are exactly 0 where the gate is 1, and at most s = sigmoid(-63.99) < 1.01 sigmoid(-64) where it is 0.
      D      = sum |dlogits| * max |W_c|: bounds every element of dL/dh_t, carried back through time by z = 1 without loss
      dpre  <= 2 D s                       (|h_prev - n| <= 2)
      b_ih, b_hh, W_hh, W_ih:  <= rows * dpre * 1.0001     (|h|, c <= 1.0001)
      de    <= colsum * dpre, colsum = the largest column sum of |W_ih|
      LayerNorm gamma / beta:  <= rows * de * 1.0001
      dy    <= rstd * de * (1 + 1 + c^2) <= 6.01 de        (rstd = 1 / sqrt(1/4 + eps) < 2)
      layer1 weight / bias:    <= rows * dy
    the largest is the last one; the factor 2 in front covers the 1.01 and the second-order term (dpre W_hh fed back into dh)."""
    D = float(dlogits.abs().sum()) * float(sd["f_classification.0.weight"].abs().max())
    colsum = float(sd["gru.weight_ih_l0"].abs().sum(dim=0).max())
    return 2.0 * rows * 6.01 * colsum * 2.0 * D


def sigmoid64(x):
    return 1.0 / (1.0 + math.exp(-x)) if x > -700 else 0.0


# ---- the runs of tests/test_gpu_automaton.py: (case, clip lengths, feature seed, options) by id; tests/test_gru_automaton_cpu.py proves
# on the CPU that each of them stays inside conditions() ------------------------------------------------------------------------------
def ragged_lens(n, lo, hi, seed, extra=()):
    g = torch.Generator().manual_seed(seed)
    return [int(x) for x in torch.randint(lo, hi + 1, (n,), generator=g)] + list(extra)


RGB, FLOW = dict(d_rgb=2048, d_flow=0), dict(d_rgb=1024, d_flow=1024)
RUNS = {}


def _add(rid, case, lens, seed=0, **opt):
    RUNS[rid] = dict(case=case, lens=lens, seed=seed, **opt)


for _hid, _C in ((1024, 12), (512, 22), (2048, 37)):
    for _name, _dims in (("rgb", RGB), ("flow", FLOW)):
        _add(f"h{_hid}-{_name}", Case(hid=_hid, n_classes=_C, emb=2048 if _hid != 512 else 1024, seed=_hid // 512, **_dims),
             ragged_lens(40, 3, 40, 5, [300]), seed=1)
_add("l2-h1024-rgb", Case(hid=1024, num_layers=2, seed=11, **RGB), ragged_lens(40, 3, 40, 6, [300]), seed=2)
_add("l2-h512-flow", Case(hid=512, emb=1024, n_classes=22, num_layers=2, seed=12, **FLOW), ragged_lens(40, 3, 40, 7, [300]), seed=3)
for _n in (40, 200, 400, 700):
    _add(f"clips{_n}", Case(seed=20, **RGB), ragged_lens(_n, 3, 40, 30 + _n, [120]), seed=4)
_add("chain", Case(seed=21, **RGB), ragged_lens(24, 20, 60, 41), seed=5, hostile_h0=True)
_add("chain-l2", Case(num_layers=2, seed=22, **RGB), ragged_lens(24, 20, 60, 42), seed=6, hostile_h0=True)
_add("long31114", Case(seed=23, **RGB), [31114], seed=7, big=True)
_add("split64", Case(seed=24, **RGB), ragged_lens(64, 4100, 4400, 51), seed=8, big=True)
_add("split50-flow", Case(d_rgb=2048, d_flow=2048, emb=2048, seed=25), ragged_lens(50, 5300, 5600, 52), seed=9, big=True)
_add("split52-e1024", Case(d_rgb=1088, d_flow=576, emb=1024, seed=26), ragged_lens(52, 5100, 5400, 53), seed=10, big=True)
_add("stream16", Case(seed=27, **RGB), [50] * 16, seed=11)
for _L in (1, 4, 8):
    _add(f"ant{_L}", Case(ant_len=_L, seed=30 + _L, **RGB), ragged_lens(30, 3, 40, 60 + _L, [200]), seed=12)
_add("train", Case(seed=40, **RGB), [128] * 16, seed=13, balanced=True)
_add("prob", Case(head_scale=1.0 / 32, seed=41, **RGB), ragged_lens(40, 3, 40, 71, [300]), seed=14, max_spread=60.0)
_add("prob-ant4", Case(head_scale=1.0 / 32, ant_len=4, seed=42, **RGB), ragged_lens(30, 3, 40, 72, [200]), seed=15, max_spread=60.0)


def hostile_h0(case: Case, n, seed):
    g = torch.Generator().manual_seed(9000 + seed)
    shape = (n, case.hid) if case.num_layers == 1 else (case.num_layers, n, case.hid)
    return torch.randint(-1, 2, shape, generator=g).to(torch.float32)


def reference(rid, device="cpu"):
    """(case, sd, meta, feats, h0, Result) of a run, conditions() checked"""
    r = RUNS[rid]
    case = r["case"]
    sd, meta = build_state_dict(case)
    # the large runs draw their bits with the device's generator; every other run draws them on the CPU, so that the CPU-only proof of
    # its conditions is about the very inputs the GPU test uses
    feats = build_features(case, r["lens"], r["seed"], device if r.get("big") else "cpu", balanced=r.get("balanced", False), sigma=meta["sigma"])
    feats = [tuple(None if t is None else t.to(device) for t in rf) for rf in feats]
    h0 = hostile_h0(case, len(r["lens"]), r["seed"]) if r.get("hostile_h0") else None
    res = run(sd, meta, case, feats, h0=h0, device=device)
    conditions(sd, case, res, max_spread=r.get("max_spread"))
    return case, sd, meta, feats, h0, res


def gate_points():
    """fp32 arguments of the gate-function sweeps: 0 and -0, +-2^-k down to the smallest subnormal, a grid of 1/64 on [-20, 20], the
    neighbours of +-17.33 (where 1 + exp(-x) starts to round to 1), +-44 (the same for tanhf_'s doubled argument near exp's range),
    the neighbours of +-88.72 (exp overflows / underflows), larger arguments and fp16's largest number"""
    pts = [0.0, -0.0]
    pts += [s * 2.0 ** -k for k in range(0, 150) for s in (1.0, -1.0)]
    pts += list(np.arange(-20.0, 20.0 + 1e-9, 1.0 / 64))
    for c in (17.33, 17.328679, 8.664339, 44.0, 44.361419, 87.336544, 88.722839, 88.7, 103.972):
        v = np.float32(c)
        lo = hi = v
        for _ in range(8):
            lo, hi = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))
            pts += [float(lo), float(hi), -float(lo), -float(hi)]
        pts += [float(v), -float(v)]
    pts += [s * v for v in (32.0, 64.0, 89.0, 100.0, 128.0, 1000.0, 65504.0) for s in (1.0, -1.0)]
    return np.asarray(pts, np.float64).astype(np.float32)
