"""float64 restatement of the recurrent layer  --  TEST INFRASTRUCTURE ONLY (used by test_rnn_regimes*.py).

Plain numpy, forward and backward of the bias-free LSTM / GRU / tanh layer of include/ctcn.h: 1 or 2 directions, zero initial state, no
packing.  Equations and gate order: SURVEY.md Appendix A (LSTM i f g o; GRU r z n with n = tanh(a_n + r * (W_hn h))).

Besides y, dx and the weight gradients it returns the two RESERVES in the layout ctcn.h documents, because they are contract (the backward
pass, ctcn_rnn_bwd_weights and a caller that defers the weight gradients all read them):

  after forward    act   (T,B,dirs,G*H)   the saved activations, gate blocks in the order above.  (The tanh cell saves nothing there: its
                                          kernels leave the input projection in `gates` and read h from y; `act` then holds h.)
                   aux   (T,B,dirs,H)     LSTM: c_t.  GRU: W_hn h_{t-1} (without r).  tanh: unused.
  after backward   da    (T,B,dirs,G*H)   d(pre-activation) as the kernels leave it in `gates`.  For the GRU the n block is
                                          dan = d(a_n + r * W_hn h), the gradient the INPUT projection receives (dx, dW_in); rnn.hip keeps
                                          that one in `gates` (rnn_bwd_step: "dan stays here, dan * r goes to aux") ...
                   daux  (T,B,dirs,H)     ... and dan * r, the gradient of W_hn h (what dW_hn and the next step's dh multiply), in `aux`.
                                          LSTM: aux is not written by the backward pass (still c_t).

`pre` (T,B,dirs,G*H) are the arguments of the gate non-linearities (GRU n block: a_n + r * W_hn h): what the saturation conditions of
test_rnn_regimes_host.py count.

The second half holds the regime generators and the designed sweep inputs, so that the host tests (which check the regimes' stated
conditions) and the GPU tests draw identical tensors.
"""
import numpy as np

CELLS = {"lstm": 0, "gru": 1, "tanh": 2}
GATES = {"lstm": 4, "gru": 3, "tanh": 1}
TORCH_NAME = {"lstm": "LSTM", "gru": "GRU", "tanh": "RNN"}


def sigmoid(a):
    """1 / (1 + exp(-a)) in float64 without overflow: exp is only ever taken of a non-positive number."""
    a = np.asarray(a, dtype=np.float64)
    e = np.exp(-np.abs(a))
    return np.where(a >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def _steps(T, d):
    """time indices in processing order: direction 1 walks t = T-1 .. 0"""
    return range(T) if d == 0 else range(T - 1, -1, -1)


def forward(cell, x, w_ih, w_hh):
    """x (T,B,I); w_ih[d] (G*H,I), w_hh[d] (G*H,H) per direction.  Returns a dict: y (T,B,dirs*H), act, aux, pre (module docstring)."""
    x = np.asarray(x, dtype=np.float64)
    T, B, _ = x.shape
    D, G, H = len(w_ih), GATES[cell], w_hh[0].shape[1]
    y = np.zeros((T, B, D, H))
    act, pre, aux = np.zeros((T, B, D, G * H)), np.zeros((T, B, D, G * H)), np.zeros((T, B, D, H))
    for d in range(D):
        wi, wh = np.asarray(w_ih[d], dtype=np.float64), np.asarray(w_hh[d], dtype=np.float64)
        gx = x.reshape(T * B, -1).dot(wi.T).reshape(T, B, G * H)
        h, c = np.zeros((B, H)), np.zeros((B, H))
        for t in _steps(T, d):
            gh = h.dot(wh.T)
            if cell == "lstm":
                a = gx[t] + gh
                i, f, g, o = sigmoid(a[:, :H]), sigmoid(a[:, H:2 * H]), np.tanh(a[:, 2 * H:3 * H]), sigmoid(a[:, 3 * H:])
                c = f * c + i * g
                h = o * np.tanh(c)
                act[t, :, d], aux[t, :, d] = np.concatenate([i, f, g, o], axis=1), c
            elif cell == "gru":
                hn = gh[:, 2 * H:]
                a = gx[t].copy()
                a[:, :2 * H] += gh[:, :2 * H]
                r, z = sigmoid(a[:, :H]), sigmoid(a[:, H:2 * H])
                a[:, 2 * H:] += r * hn
                n = np.tanh(a[:, 2 * H:])
                h = (1.0 - z) * n + z * h
                act[t, :, d], aux[t, :, d] = np.concatenate([r, z, n], axis=1), hn
            else:
                a = gx[t] + gh
                h = np.tanh(a)
                act[t, :, d] = h
            pre[t, :, d], y[t, :, d] = a, h
    return {"y": y.reshape(T, B, D * H), "act": act, "aux": aux, "pre": pre}


def backward(cell, x, w_ih, w_hh, fwd, dy):
    """The backward pass of `forward` for the output gradient dy (T,B,dirs*H).  Returns a dict: dx (T,B,I), dw_ih[d], dw_hh[d], da, daux."""
    x, dy = np.asarray(x, dtype=np.float64), np.asarray(dy, dtype=np.float64)
    T, B, I = x.shape
    D, G, H = len(w_ih), GATES[cell], w_hh[0].shape[1]
    y, act, aux = fwd["y"].reshape(T, B, D, H), fwd["act"], fwd["aux"]
    dy = dy.reshape(T, B, D, H)
    da, dah, daux = np.zeros((T, B, D, G * H)), np.zeros((T, B, D, G * H)), np.zeros((T, B, D, H))
    dx, dw_ih, dw_hh = np.zeros((T * B, I)), [], []
    zero = np.zeros((B, H))
    for d in range(D):
        wi, wh = np.asarray(w_ih[d], dtype=np.float64), np.asarray(w_hh[d], dtype=np.float64)
        order = list(_steps(T, d))
        dh_rec, carry = np.zeros((B, H)), np.zeros((B, H))          # d(pre-act)_{next} W_hh;  dc (LSTM) / dh * z (GRU)
        hprev = np.zeros((T, B, H))
        for k in range(T - 1, -1, -1):
            t = order[k]
            tp = order[k - 1] if k > 0 else None
            hp = y[tp, :, d] if tp is not None else zero
            hprev[t] = hp
            dh = dy[t, :, d] + dh_rec
            if cell == "lstm":
                i, f, g, o = (act[t, :, d, j * H:(j + 1) * H] for j in range(4))
                cp = aux[tp, :, d] if tp is not None else zero
                tc = np.tanh(aux[t, :, d])
                dc = dh * o * (1.0 - tc * tc) + carry
                blocks = [dc * g * i * (1.0 - i), dc * cp * f * (1.0 - f), dc * i * (1.0 - g * g), dh * tc * o * (1.0 - o)]
                carry = dc * f
                da[t, :, d] = dah[t, :, d] = np.concatenate(blocks, axis=1)
            elif cell == "gru":
                r, z, n = (act[t, :, d, j * H:(j + 1) * H] for j in range(3))
                hn = aux[t, :, d]
                dh = dh + carry
                dan = dh * (1.0 - z) * (1.0 - n * n)
                dar, daz = dan * hn * r * (1.0 - r), dh * (hp - n) * z * (1.0 - z)
                carry = dh * z
                da[t, :, d] = np.concatenate([dar, daz, dan], axis=1)
                dah[t, :, d] = np.concatenate([dar, daz, dan * r], axis=1)
                daux[t, :, d] = dan * r
            else:
                h = y[t, :, d]
                da[t, :, d] = dah[t, :, d] = dh * (1.0 - h * h)
            dh_rec = dah[t, :, d].dot(wh)
        a2 = da[:, :, d].reshape(T * B, G * H)
        dx += a2.dot(wi)
        dw_ih.append(a2.T.dot(x.reshape(T * B, I)))
        dw_hh.append(dah[:, :, d].reshape(T * B, G * H).T.dot(hprev.reshape(T * B, H)))
    if cell == "lstm":
        daux = aux.copy()
    return {"dx": dx.reshape(T, B, I), "dw_ih": dw_ih, "dw_hh": dw_hh, "da": da, "daux": daux}


def run(cell, case):
    """forward + backward of a case of `make_case` / `sweep_case`: one dict with everything."""
    out = forward(cell, case["x"], case["w_ih"], case["w_hh"])
    out.update(backward(cell, case["x"], case["w_ih"], case["w_hh"], out, case["dy"]))
    return out


def rel_l2(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm((a - b).ravel()) / max(np.linalg.norm(b.ravel()), 1e-300))


def max_abs(a, b):
    return float(np.max(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64))))


# ---------------------------------------------------------------------------------------------------------------------------------
# The trained-model regimes.  A torch-default-initialised layer (U(+-1/sqrt(H)), drawn by torch itself from `seed`), W_hh untouched:
# scaling W_hh as well gives a chaotic layer (|dx| 1e8-1e10 at H = 320, T = 24; torch f32 100 % away from torch f64), about which
# nothing can be asserted.  Saturation comes in through the input projection:
#   input16 / input64   W_ih * 16 / * 64 (powers of two: exact in f32)
#   mixed               row r of W_ih * g_r, g_r log-uniform in [0.25, 64]: linear, half-saturated and fully saturated units side by side
#                       in every 16-unit slice
#   memory (LSTM, GRU)  input feature 0 is the constant 1 and column 0 of W_ih is 0 except on the forget (LSTM) / update (GRU) rows, where
#                       it is U(2, 8): a per-unit bias that keeps state for tens to thousands of frames.  For the LSTM the other
#                       features are speech-like -- a per-utterance offset (MEMORY_OFFSET * randn, constant over time) plus unit noise --
#                       so that the candidate keeps its sign over the sequence and c really integrates (|c| >= 3; with white noise alone
#                       the long-lived cell has nothing to remember: |c| stays below 1 at H = 320).  The GRU's state is bounded by 1
#                       whatever it is fed and keeps the white input: with the offset torch's own float32 dx sits AT the 5e-6 no-chaos
#                       cap (4.9-5.5e-6: 1 - z of a saved z = 0.997 has five digits left), which leaves nothing to assert against.
# ---------------------------------------------------------------------------------------------------------------------------------
REGIMES = ("input16", "input64", "mixed", "memory")
MEMORY_OFFSET = 3.0
# (T, B, I, H): the smallest shapes that reach each code path of rnn.hip (why: test_rnn_regimes.py)
SHAPES = ((48, 5, 8, 32), (48, 17, 16, 72), (24, 9, 16, 320), (24, 9, 16, 384), (12, 33, 8, 512))
CHUNK_SHAPE = (12, 144, 16, 320)            # the batch-chunk case (memory, LSTM)
# `mixed` at H = 512: with I = 8 only 3 % of the pre-activations pass |a| = 4 (std of a row = g_r sqrt(I / 3H)), short of the regime's 5 %;
# I = 32 gives 10 %.  The recurrence kernels never see I (it is the projection GEMM's K).
MIXED_WIDE = (12, 33, 32, 512)


def regimes_of(cell):
    return REGIMES if cell != "tanh" else REGIMES[:3]


def layer_cases():
    """Every (cell, regime, T, B, I, H, dirs) the GPU tests run -- the host tests hold each of them to its regime's conditions first."""
    cases = [(cell, regime) + (MIXED_WIDE if (regime, shape) == ("mixed", SHAPES[4]) else shape) + (2,)
             for shape in SHAPES for cell in ("lstm", "gru") for regime in REGIMES]
    cases += [("tanh", regime) + shape + (2,) for shape in SHAPES[:2] for regime in regimes_of("tanh")]
    cases += [("lstm", "mixed") + SHAPES[0] + (1,), ("gru", "memory") + SHAPES[1] + (1,)]
    return cases + [("lstm", "memory") + CHUNK_SHAPE + (2,)]


_cache = {}


def layer_case(key):
    """(case, float64 reference) of a `layer_cases` entry: computed once per process, shared by every test, never written to."""
    if key not in _cache:
        cell, regime, T, B, I, H, dirs = key
        case = make_case(cell, regime, T, B, I, H, dirs)
        ref = run(cell, case)
        for a in list(case.values()) + list(ref.values()):
            for arr in (a if isinstance(a, list) else [a]):
                arr.setflags(write=False)
        _cache[key] = (case, ref)
    return _cache[key]


def make_case(cell, regime, T, B, I, H, dirs=2, seed=0):
    """{x, dy, w_ih[d], w_hh[d]}: float32 arrays (what the GPU gets; the references take them up to float64 unchanged)."""
    import torch
    g = torch.Generator().manual_seed(1000 * seed + 17 * H + T + B)
    G = GATES[cell]
    k = 1.0 / H ** 0.5
    w_ih = [((torch.rand(G * H, I, generator=g) * 2 - 1) * k).numpy() for _ in range(dirs)]
    w_hh = [((torch.rand(G * H, H, generator=g) * 2 - 1) * k).numpy() for _ in range(dirs)]
    x = torch.randn(T, B, I, generator=g).numpy()
    dy = torch.randn(T, B, dirs * H, generator=g).numpy()
    if regime in ("input16", "input64"):
        w_ih = [w * np.float32(int(regime[5:])) for w in w_ih]
    elif regime == "mixed":
        for d in range(dirs):
            gain = np.exp(torch.rand(G * H, generator=g).numpy().astype(np.float64) * np.log(64 / 0.25) + np.log(0.25))
            w_ih[d] = (w_ih[d] * gain[:, None]).astype(np.float32)
    elif regime == "memory":
        assert cell in ("lstm", "gru")
        if cell == "lstm":
            x = x + MEMORY_OFFSET * torch.randn(1, B, I, generator=g).numpy()
        x[:, :, 0] = 1.0
        for d in range(dirs):
            w_ih[d][:, 0] = 0.0
            w_ih[d][H:2 * H, 0] = (2.0 + 6.0 * torch.rand(H, generator=g)).numpy()      # block 1: f (LSTM) / z (GRU)
    else:
        raise ValueError(regime)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return {"x": f32(x), "dy": f32(dy), "w_ih": [f32(w) for w in w_ih], "w_hh": [f32(w) for w in w_hh]}


def torch_layer(cell, case, dtype):
    """torch.nn.LSTM / GRU / RNN (bias=False) with the case's weights, forward and backward in `dtype` on the CPU:
    {y, dx, dw_ih[d], dw_hh[d]} as float64 numpy."""
    import torch
    dirs, H, I = len(case["w_ih"]), case["w_hh"][0].shape[1], case["x"].shape[2]
    m = getattr(torch.nn, TORCH_NAME[cell])(I, H, bidirectional=dirs == 2, bias=False).to(dtype)
    sfx = ["", "_reverse"]
    with torch.no_grad():
        for d in range(dirs):
            getattr(m, "weight_ih_l0" + sfx[d]).copy_(torch.tensor(case["w_ih"][d], dtype=dtype))
            getattr(m, "weight_hh_l0" + sfx[d]).copy_(torch.tensor(case["w_hh"][d], dtype=dtype))
    x = torch.tensor(case["x"], dtype=dtype).requires_grad_(True)
    y, _ = m(x)
    y.backward(torch.tensor(case["dy"], dtype=dtype))
    n64 = lambda t: t.detach().double().numpy()
    return {"y": n64(y), "dx": n64(x.grad), "dw_ih": [n64(getattr(m, "weight_ih_l0" + sfx[d]).grad) for d in range(dirs)],
            "dw_hh": [n64(getattr(m, "weight_hh_l0" + sfx[d]).grad) for d in range(dirs)]}


def gradients(out):
    """[(name, array)] of dx and the weight gradients of a result dict"""
    res = [("dx", out["dx"])]
    for d in range(len(out["dw_ih"])):
        res += [("dw_ih%d" % d, out["dw_ih"][d]), ("dw_hh%d" % d, out["dw_hh"][d])]
    return res


def saturated_share(pre, bound=4.0):
    return float(np.mean(np.abs(pre) > bound))


# ---------------------------------------------------------------------------------------------------------------------------------
# The pointwise sweep: designed inputs whose pre-activations are known exactly.
# I = G; W_ih[g*H + j, g] = s_j = 2^(j mod 9 - 4) and zero elsewhere, so a_g[t,b,j] = s_j * x[t,b,g]: one product with a power of two, exact
# in f32 and -- x rounded to 12 significant bits, i.e. to two bf16 planes at most -- in the bf16x3 split.
# ---------------------------------------------------------------------------------------------------------------------------------
SWEEP_MAGNITUDES = (2.0 ** -20, 1e-3, 0.1, 0.5, 1.0, 2.0, 4.0, 5.5, 8.0, 16.0, 32.0, 64.0, 87.0, 89.0, 104.0, 1000.0, 3e38)


def round_bits(v, bits=12):
    """v rounded to `bits` significant bits (float64 in, exactly representable in float32 out)"""
    v = np.asarray(v, dtype=np.float64)
    m, e = np.frexp(v)
    return np.ldexp(np.round(m * 2.0 ** bits) / 2.0 ** bits, e)


def sweep_grid():
    """{0, -0, +-m for m in SWEEP_MAGNITUDES}, each rounded to 12 significant bits, as float32"""
    mags = round_bits(np.array(SWEEP_MAGNITUDES))
    grid = np.concatenate([[0.0, -0.0], mags, -mags]).astype(np.float32)
    assert np.all(np.isfinite(grid)) and np.array_equal(grid.astype(np.float64)[2:], np.concatenate([mags, -mags]))
    return grid


def sweep_scales(H):
    return 2.0 ** ((np.arange(H) % 9) - 4.0)


def sweep_arguments():
    """Every pre-activation the sweep can produce (grid x scales), float64: the grid the host test walks the activation formulas over."""
    g = sweep_grid().astype(np.float64)
    a = (g[:, None] * sweep_scales(9)[None, :]).ravel()
    return a[np.abs(a) <= np.finfo(np.float32).max]


def sweep_case(cell, H, whh_scale, T=3, B=64, dirs=2, seed=0):
    """The designed layer.  whh_scale: 0.0 (recurrent sums exactly 0) or 0.5 (0.5 * I in every gate block).  x: B rows of random grid
    combinations.  All INPUTS are finite; the product 3e38 * s_j with s_j > 1 is beyond float32 and reaches the activation as +-inf on the
    device (and as 4.8e39 here), which is the same saturated value."""
    rs = np.random.RandomState(4242 + 10 * seed + H)
    G = GATES[cell]
    grid = sweep_grid()
    x = grid[rs.randint(0, len(grid), size=(T, B, G))]
    s = sweep_scales(H)
    w_ih, w_hh = [], []
    for d in range(dirs):
        w = np.zeros((G * H, G), dtype=np.float32)
        for g_ in range(G):
            w[g_ * H:(g_ + 1) * H, g_] = s
        w_ih.append(w)
        w_hh.append(np.ascontiguousarray(np.tile(np.eye(H, dtype=np.float32) * np.float32(whh_scale), (G, 1))))
    dy = round_bits(rs.randn(T, B, dirs * H), 8).astype(np.float32)
    return {"x": np.ascontiguousarray(x), "dy": dy, "w_ih": w_ih, "w_hh": w_hh}


# ---------------------------------------------------------------------------------------------------------------------------------
# Derived per-element error bounds for the sweep (nothing here is fitted to a kernel's output).
#
# Running error analysis, first order with the second-order cross terms kept: every quantity is a pair (v, e) -- its float64 value and a
# bound on |device value - v|.  The designed layer is element-wise (W_ih has one entry per row, W_hh is a multiple of I per gate block),
# so unit j of row b depends on nothing but its own history and the pairs are plain arrays.
#   * inputs (x, dy, the weights) are exact: e = 0;  s_j * x is one product with a power of two: exact
#   * a float32 operation rounds its result:          e(a op b) = propagated error + U * |a op b|,  U = 2^-23 (one ulp; a fused
#     multiply-add rounds once instead of twice, so the bound holds for whichever contraction the compiler chose)
#       e(a + b) = e_a + e_b,   e(a * b) = |a| e_b + |b| e_a + e_a e_b
#   * an activation f (sigmoid or tanh) of an argument known to e_a: by the mean value theorem |f(a') - f(a)| <= max|f'| e_a over
#     [a - e_a, a + e_a]; both derivatives fall with |a|, so the maximum is f'(max(|a| - e_a, 0)).  On top comes the source's own claim for
#     the hardware formula, ACT_EPS = 3e-7 absolute (the comment above act_sigmoid in rnn.hip):   e = ACT_EPS + f'(...) e_a
#   * a recurrent product w * h with w = 0.5: exact in f32 (precision 0).  At precision 1 h travels as two bf16 planes, hi + lo, which
#     drops |h| 2^-16 at most (the project's figure for bf16x3): e = 0.5 e_h + SPLIT * |0.5 h|, SPLIT = 2^-16 at precision 1, else 0
#   * a sum of n such products (backward: the G gate blocks of a unit; dx: dirs * H units) adds n * U * sum|terms|
# The expressions below are those of cell_fwd / cell_bwd in rnn.hip, term for term.
# ---------------------------------------------------------------------------------------------------------------------------------
ACT_EPS = 3e-7
U = 2.0 ** -23


class Err(object):
    def __init__(self, v, e=None):
        self.v = np.asarray(v, dtype=np.float64)
        self.e = np.zeros_like(self.v) if e is None else np.asarray(e, dtype=np.float64)

    @staticmethod
    def of(o):
        return o if isinstance(o, Err) else Err(o)

    def _rounded(self, v, e):
        return Err(v, e + U * np.abs(v))

    def __add__(self, o):
        o = Err.of(o)
        return self._rounded(self.v + o.v, self.e + o.e)

    def __sub__(self, o):
        o = Err.of(o)
        return self._rounded(self.v - o.v, self.e + o.e)

    def __rsub__(self, o):
        return Err.of(o) - self

    def __mul__(self, o):
        o = Err.of(o)
        return self._rounded(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e)


def _act(a, fn, dfn):
    lo = np.maximum(np.abs(a.v) - a.e, 0.0)
    return Err(fn(a.v), ACT_EPS + dfn(lo) * a.e)


def err_sigmoid(a):
    return _act(a, sigmoid, lambda t: sigmoid(t) * (1.0 - sigmoid(t)))


def err_tanh(a):
    return _act(a, np.tanh, lambda t: 1.0 - np.tanh(t) ** 2)


def _rec(h, w, split):
    """w * h for the recurrent weight w (0 or 0.5): exact at precision 0, the bf16x3 split's loss at precision 1"""
    return Err(w * h.v, abs(w) * h.e + split * np.abs(w * h.v))


def _sum(terms):
    """a device-side sum of n terms in any order: n roundings of at most sum|terms|"""
    v = sum(t.v for t in terms)
    return Err(v, sum(t.e for t in terms) + len(terms) * U * sum(np.abs(t.v) for t in terms))


SPLIT = 2.0 ** -16
# What rnn_fwd_tagged can actually lose: hi and lo are each rounded to nearest, which leaves 2^-17 of |h| (binade bottom), and the step tag
# then replaces the LSB of lo, one ulp of lo = another 2^-16 of |h|.  The comment above the kernel counts the tag alone ("2^-16 relative").
SPLIT_TAGGED = 1.5 * 2.0 ** -16


def sweep_bounds(cell, case, precision, split_figure=SPLIT):
    """Values and bounds for the designed layer of `sweep_case`: a dict of Err with the keys act, aux, y (forward) and da, daux, dx
    (backward), shaped as the results of `run`.  Needs W_hh = w * I per gate block (w read from the case).  split_figure: what a bf16x3
    operand loses, relative (precision 1 only)."""
    x, dy = case["x"].astype(np.float64), case["dy"].astype(np.float64)
    T, B, G = x.shape
    D, H = len(case["w_ih"]), case["w_hh"][0].shape[1]
    assert G == GATES[cell]
    w = float(case["w_hh"][0][0, 0])
    split = split_figure if (precision == 1 and w != 0.0) else 0.0
    s = sweep_scales(H)
    zero = Err(np.zeros((B, H)))
    pack = lambda lst: Err(np.concatenate([t.v for t in lst], axis=-1), np.concatenate([t.e for t in lst], axis=-1))
    out = {k: [[None] * D for _ in range(T)] for k in ("act", "aux", "y", "da", "daux")}
    dx_terms = [[[] for _ in range(G)] for _ in range(T)]
    for d in range(D):
        order = list(_steps(T, d))
        h, c = zero, zero
        cs, hs = {}, {}
        for t in order:
            pre = [Err(x[t, :, g_, None] * s[None, :]) for g_ in range(G)]
            first = t == order[0]
            add = (lambda p, o: p) if (w == 0.0 or first) else (lambda p, o: o + p)      # o = +0 exactly: the sum is the projection itself
            if cell == "lstm":
                o = _rec(h, w, split)
                i_, f_, g_, o_ = err_sigmoid(add(pre[0], o)), err_sigmoid(add(pre[1], o)), err_tanh(add(pre[2], o)), err_sigmoid(add(pre[3], o))
                c = f_ * c + i_ * g_
                h = o_ * err_tanh(c)
                out["act"][t][d], out["aux"][t][d] = pack([i_, f_, g_, o_]), c
            elif cell == "gru":
                o = _rec(h, w, split)
                r_, z_ = err_sigmoid(add(pre[0], o)), err_sigmoid(add(pre[1], o))
                n_ = err_tanh(add(pre[2], r_ * o))
                h = (1.0 - z_) * n_ + z_ * h
                out["act"][t][d], out["aux"][t][d] = pack([r_, z_, n_]), o
            else:
                h = err_tanh(add(pre[0], _rec(h, w, split)))
                out["act"][t][d], out["aux"][t][d] = h, zero
            out["y"][t][d] = h
            cs[t], hs[t] = c, h
        carry, nxt = zero, None
        for k in range(T - 1, -1, -1):
            t = order[k]
            tp = order[k - 1] if k > 0 else None
            dh = Err(dy[t, :, d * H:(d + 1) * H])
            if nxt is not None and w != 0.0:
                dh = dh + _sum([_rec(o_, w, split) for o_ in nxt])
            a = out["act"][t][d]
            blk = lambda j: Err(a.v[:, j * H:(j + 1) * H], a.e[:, j * H:(j + 1) * H])
            if cell == "lstm":
                i_, f_, g_, o_ = blk(0), blk(1), blk(2), blk(3)
                tc = err_tanh(cs[t])
                dc = dh * o_ * (1.0 - tc * tc) + carry
                e1 = cs[tp] if tp is not None else zero
                nxt = [dc * g_ * i_ * (1.0 - i_), dc * e1 * f_ * (1.0 - f_), dc * i_ * (1.0 - g_ * g_), dh * tc * o_ * (1.0 - o_)]
                carry = dc * f_
                stored, out["daux"][t][d] = nxt, cs[t]
            elif cell == "gru":
                r_, z_, n_ = blk(0), blk(1), blk(2)
                hn, hp = out["aux"][t][d], (hs[tp] if tp is not None else zero)
                dh = dh + carry
                dan = dh * (1.0 - z_) * (1.0 - n_ * n_)
                nxt = [dan * hn * r_ * (1.0 - r_), dh * (hp - n_) * z_ * (1.0 - z_), dan * r_]
                carry = dh * z_
                stored, out["daux"][t][d] = [nxt[0], nxt[1], dan], nxt[2]
            else:
                stored = nxt = [dh * (1.0 - hs[t] * hs[t])]
                out["daux"][t][d] = zero
            out["da"][t][d] = pack(stored)
            for g_ in range(G):          # dx[t,b,g] = sum over directions and units of da_g[j] * s_j (s_j exact; da split at precision 1)
                dx_terms[t][g_].append(Err(stored[g_].v * s, stored[g_].e * s + (split_figure if precision == 1 else 0.0) * np.abs(stored[g_].v * s)))
    res = {}
    for k in ("act", "aux", "y", "da", "daux"):
        v = np.stack([np.stack([out[k][t][d].v for d in range(D)], axis=1) for t in range(T)])       # (T,B,D,*)
        e = np.stack([np.stack([out[k][t][d].e for d in range(D)], axis=1) for t in range(T)])
        res[k] = Err(v.reshape(T, B, -1), e.reshape(T, B, -1)) if k == "y" else Err(v, e)
    dxv, dxe = np.zeros((T, B, G)), np.zeros((T, B, G))
    for t in range(T):
        for g_ in range(G):
            v = np.concatenate([q.v for q in dx_terms[t][g_]], axis=1)
            e = np.concatenate([q.e for q in dx_terms[t][g_]], axis=1)
            dxv[t, :, g_] = v.sum(axis=1)
            dxe[t, :, g_] = e.sum(axis=1) + v.shape[1] * U * np.abs(v).sum(axis=1)
    res["dx"] = Err(dxv, dxe)
    return res
