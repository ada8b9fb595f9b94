"""The fused GRU cell step (shifu_amd/csrc/shf_gru.hip) and the recurrent policy on it, against float64 torch on the CPU.

Forward bound (derived).  The GEMM's pre-activations a_r + b, a_z + b, a_nx + b_in and hn = a_nh + b_hn each
carry an error of at most e = tmax * S (tmax: TOL of tests/test_gpu_mlp.py for the operand precision; S: the largest
magnitude among the four in the float64 reference).  Then
    sigma' <= 1/4                      |dr|, |dz| <= e/4
    n's argument a_nx + b_in + r hn    errs by at most e + |r| e + |hn| |dr| <= (2 + max|hn|/4) e;  tanh' <= 1 gives |dn|
    h' = (1 - z) n + z he              |dh'| <= |dn| + (|he| + |n|) |dz| <= (2.25 + max|hn|/4 + max|h_prev|/4) e
The kept gates (r, z, n, hn) are checked with the per-gate parts: e/4, e/4, (2 + max|hn|/4) e, e.  The fp32 pointwise
arithmetic adds an absolute term: the same formulas evaluated by torch in fp32 on the GPU from the float64 pre-activations
differ from float64 by at most POINTWISE_FP32 on these inputs (measured, printed by the test); four times that is allowed
for another exp form.  The kernel's own output equals (1 - z) * n + z * he evaluated in fp32 from its kept gates bit for
bit (no contraction), which the forward test checks as well.

The r pin's bound.  With b_ir = -40 and no r weights r <= 2^-57, so r hn and r's share of n's error vanish against fp32
and n's argument carries the n_x accumulator's error alone: tmax * max|a_nx + b_in|.  With b_ir = +40, r = 1 exactly
(1 + exp(-40) rounds to 1), dr = 0, and the argument carries both accumulators' errors: tmax * (max|a_nx + b_in| +
max|hn|).  Both are inside the forward bound above, which is asserted too; they are what makes the pin sharp under bf16
operands, where S >= 40 makes the general bound wider than tanh's range.

Backward ceilings: one step 4 x TOL of each tensor's scale (the forward gates, the kept hn that multiplies into dr, the
derivative evaluated at them, the gradient GEMM); a sequence: the number of GEMMs chained on the longest path x TOL."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from tests.test_gpu_mlp import TOL      # noqa: E402

DEV = "cuda:0"
SHAPES = [(1, 5, 32), (33, 5, 40), (70, 19, 96), (37, 33, 6), (64, 259, 512)]
PINS = SHAPES[:2]
# max |fp32 torch pointwise - float64| over h', r, z, n, hn and the inputs of test_forward_matches_float64, measured on an
# MI355X: 1.86e-7 (h', at (64, 259, 512)); r 8.13e-8, z 7.75e-8, n 1.29e-7, hn (the fp32 rounding of its value) 5.95e-8
POINTWISE_FP32 = 1.86e-7


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible")


@pytest.fixture(params=["bf16x3", "bf16"])
def precision(request):
    from shifu_amd.rl import mfma_linear
    _need_gpu()
    before = mfma_linear.get_precision()
    mfma_linear.set_precision(request.param)
    yield request.param
    mfma_linear.set_precision(before)


def _weights(I, H, seed):
    g = torch.Generator().manual_seed(seed)
    k = 1.0 / np.sqrt(H)
    u = lambda *s: (torch.rand(*s, generator=g, dtype=torch.float64) * 2 - 1) * k      # nn.GRU's initialisation
    return [u(3 * H, I), u(3 * H, H), u(3 * H), u(3 * H)]


def _inputs(M, I, H, seed, with_reset):
    g = torch.Generator().manual_seed(seed + 100)
    x = torch.randn(M, I, generator=g, dtype=torch.float64) * 1.5
    h = torch.randn(M, H, generator=g, dtype=torch.float64) * 0.5
    reset = None
    if with_reset:
        reset = (torch.rand(M, generator=g) < 0.4).to(torch.uint8)
        reset[0] = 1
    return x, h, reset


def _keep(reset, like):
    return torch.ones(like.shape[0], 1, dtype=like.dtype, device=like.device) if reset is None else (1.0 - reset.to(like.device, like.dtype)).unsqueeze(1)


def _pointwise(pr, pz, pnx, hn, he):
    """The cell's pointwise update from the (biased) pre-activations, in the dtype and on the device of its arguments."""
    r, z = torch.sigmoid(pr), torch.sigmoid(pz)
    n = torch.tanh(pnx + r * hn)
    return (1 - z) * n + z * he, r, z, n


def _ref_cell(x, h, reset, w_ih, w_hh, b_ih, b_hh):
    """float64: h', and pre = (a_r + b, a_z + b, a_nx + b_in, hn, he), reset by multiplication."""
    H = h.shape[1]
    he = h * _keep(reset, h)
    gx, gh = x @ w_ih.t() + b_ih, he @ w_hh.t() + b_hh
    pre = (gx[:, :H] + gh[:, :H], gx[:, H:2 * H] + gh[:, H:2 * H], gx[:, 2 * H:], gh[:, 2 * H:], he)
    return _pointwise(*pre)[0], pre


def _f32(*ts):
    return [None if t is None else (t.to(DEV) if t.dtype == torch.uint8 else t.detach().to(DEV, torch.float32)) for t in ts]


def _raw_cell(x, ldx, h, reset, w, M, I, H, want_gates=True):
    """The C entries directly: pack, then one cell step; x is read through the row stride ldx."""
    from shifu_amd._lib import lib
    L = lib()
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    nb = C.c_int64()
    assert L.shf_gru_pack_bytes(I, H, C.byref(nb)) == 0
    pack = torch.empty(nb.value, device=DEV, dtype=torch.uint8)
    assert L.shf_gru_pack_weights(p(w[0]), p(w[1]), p(pack), I, H, st) == 0, L.shf_mlp_last_error()
    ho = torch.full((M, H), 7.0, device=DEV)
    gates = torch.full((M, 4 * H), 9.0, device=DEV) if want_gates else None
    rc = L.shf_gru_cell_forward(p(x), ldx, p(h), p(reset), p(pack), p(w[2]), p(w[3]), p(ho), p(gates), M, I, H, st)
    assert rc == 0, L.shf_mlp_last_error()
    return ho, gates


def _errs(ho, gates, h_ref, pre):
    """max |error| of h', r, z, n, hn against the float64 reference."""
    _, r, z, n = _pointwise(*pre)
    got = [ho.cpu().double()] + list(gates.cpu().double().chunk(4, dim=1))
    return [float((a - b).abs().max()) for a, b in zip(got, [h_ref, r, z, n, pre[3]])]


def _bounds(precision, pre, h):
    """(bounds of h', r, z, n, hn; S) of the module docstring."""
    S = max(float(p.abs().max()) for p in pre[:4])
    e = TOL[precision][0] * S
    hn, pw = float(pre[3].abs().max()), 4 * POINTWISE_FP32
    return [(2.25 + hn / 4 + float(h.abs().max()) / 4) * e + pw, e / 4 + pw, e / 4 + pw, (2 + hn / 4) * e + pw, e + pw], S


def _consistent(ho, gates, h, reset):
    """h' is (1 - z) * n + z * he of the kept gates, bit for bit."""
    r, z, n, hn = gates.cpu().chunk(4, dim=1)
    he = h.cpu() * _keep(reset, h).cpu()
    return torch.equal(ho.cpu(), (1 - z) * n + z * he)


@pytest.mark.parametrize("with_reset", [False, True])
@pytest.mark.parametrize("M,I,H", SHAPES)
def test_forward_matches_float64(M, I, H, with_reset, precision):
    _need_gpu()
    w = _weights(I, H, seed=M + H)
    x, h, reset = _inputs(M, I, H, seed=M, with_reset=with_reset)
    h_ref, pre = _ref_cell(x, h, reset, *w)
    ho, gates = _raw_cell(*_f32(x), I, *_f32(h, reset), _f32(*w), M, I, H)
    # the absolute term: torch's fp32 pointwise formulas on the GPU from the same pre-activations, against float64
    p32 = _f32(*pre)
    out32 = _pointwise(*p32)
    ref64 = _pointwise(*pre)
    pw = [float((a.cpu().double() - b).abs().max()) for a, b in zip(out32, ref64)] + [float((p32[3].cpu().double() - pre[3]).abs().max())]
    bounds, S = _bounds(precision, pre, h)
    errs = _errs(ho, gates, h_ref, pre)
    names = ["h'", "r", "z", "n", "hn"]
    print(f"gru forward {(M, I, H)} reset={with_reset} [{precision}]: " +
          ", ".join(f"{n} {e:.3g} (bound {b:.3g})" for n, e, b in zip(names, errs, bounds)) +
          f"; torch fp32 pointwise vs float64: h' {pw[0]:.3g}, r {pw[1]:.3g}, z {pw[2]:.3g}, n {pw[3]:.3g}, hn {pw[4]:.3g} "
          f"(max {max(pw):.3g}, POINTWISE_FP32 {POINTWISE_FP32:.3g}); S {S:.3g}")
    for n, e, b in zip(names, errs, bounds):
        assert e <= b, n
    assert _consistent(ho, gates, *_f32(h, reset))
    if with_reset:      # a finished row does not see its h_prev at all
        h2 = h.clone()
        h2[reset.bool()] = 123.0
        ho2, _ = _raw_cell(*_f32(x), I, *_f32(h2, reset), _f32(*w), M, I, H)
        assert torch.equal(ho2, ho)


@pytest.mark.parametrize("M,I,H", PINS)
def test_z_pin_returns_h_prev_bitwise(M, I, H, precision):
    """b_iz = +40 and no z weights on every third unit: z = 1 exactly there, so h' is rho h_prev bit for bit -- the z tile, the
    unit index and the reset factor of the epilogue's h_prev read cannot be in the wrong place."""
    _need_gpu()
    w = _weights(I, H, seed=3)
    x, h, reset = _inputs(M, I, H, seed=4, with_reset=True)
    pin = torch.arange(H) % 3 == 0
    w[0][H:2 * H][pin] = 0.0
    w[1][H:2 * H][pin] = 0.0
    w[2][H:2 * H][pin] = 40.0
    xd, hd, rd = _f32(x, h, reset)
    ho, gates = _raw_cell(xd, I, hd, rd, _f32(*w), M, I, H)
    want = hd * _keep(rd, hd)
    assert torch.equal(ho[:, pin.to(DEV)], want[:, pin.to(DEV)])
    assert (gates[:, H:2 * H][:, pin.to(DEV)] == 1.0).all()
    free = ~pin
    assert not torch.equal(ho[:, free.to(DEV)], want[:, free.to(DEV)])          # (the other units do move)
    h_ref, pre = _ref_cell(x, h, reset, *w)
    for name, e, b in zip(["h'", "r", "z", "n", "hn"], _errs(ho, gates, h_ref, pre), _bounds(precision, pre, h)[0]):
        assert e <= b, name


@pytest.mark.parametrize("M,I,H", PINS)
def test_r_pin_keeps_the_h_half_of_the_n_tile_out_of_n_x(M, I, H, precision):
    """b_ir = -40 without r weights and W_hn entries of magnitude 50: n must be tanh(x W_in^T + b_in) -- the h half of the n
    tile, had it leaked into n_x, would saturate n.  b_ir = +40 then gives the full sum.  Bounds: the module docstring."""
    _need_gpu()
    w = _weights(I, H, seed=5)
    g = torch.Generator().manual_seed(6)
    x, h, reset = _inputs(M, I, H, seed=7, with_reset=M > 1)
    h = h * 0.1
    w[0][:H] = 0.0
    w[1][:H] = 0.0
    w[1][2 * H:] = 50.0 * (torch.randint(0, 2, (H, H), generator=g).double() * 2 - 1)
    tmax, pw = TOL[precision][0], 4 * POINTWISE_FP32
    for b_ir in (-40.0, 40.0):
        w[2][:H] = b_ir
        h_ref, pre = _ref_cell(x, h, reset, *w)
        ho, gates = _raw_cell(*_f32(x), I, *_f32(h, reset), _f32(*w), M, I, H)
        errs, (bounds, S) = _errs(ho, gates, h_ref, pre), _bounds(precision, pre, h)
        s_nx, s_hn = float(pre[2].abs().max()), float(pre[3].abs().max())
        n_ref = _pointwise(*pre)[3]
        if b_ir < 0:
            n_only_x = torch.tanh(x @ w[0][2 * H:].t() + w[2][2 * H:])
            assert float((n_ref - n_only_x).abs().max()) <= 1e-14               # the reference itself: r hn is gone
            assert float((torch.tanh(pre[2] + pre[3]) - n_only_x).abs().max()) > 0.5          # ... and a leak would show
            sharp = tmax * s_nx + pw
        else:
            assert (gates[:, :H] == 1.0).all()
            assert float((n_ref - torch.tanh(pre[2] + pre[3])).abs().max()) <= 1e-14
            sharp = tmax * (s_nx + s_hn) + pw
        print(f"gru r pin {(M, I, H)} b_ir={b_ir:+.0f} [{precision}]: n err {errs[3]:.3g} (sharp bound {sharp:.3g}, forward bound {bounds[3]:.3g}), "
              f"h' err {errs[0]:.3g} (bound {bounds[0]:.3g}); max|a_nx + b| {s_nx:.3g}, max|hn| {s_hn:.3g}, S {S:.3g}")
        assert errs[3] <= sharp and sharp <= bounds[3]
        for name, e, b in zip(["h'", "r", "z", "n", "hn"], errs, bounds):
            assert e <= b, name


@pytest.mark.parametrize("M,I,H", PINS)
def test_one_hot_rows_pin_the_k_index(M, I, H, precision):
    """One-hot x rows at k = 0 and I - 1, one-hot h rows at 0 and H - 1, weights that are signed powers of two (bf16-exact), no
    bias: every pre-activation is one weight, exactly, on both sides of x's padding.  hn is checked bit for bit, r, z, n to the
    fp32 pointwise term, h' against the kept gates bit for bit."""
    _need_gpu()
    rows = max(M, 4)
    pat = torch.arange(rows) % 4
    x, h = torch.zeros(rows, I, dtype=torch.float64), torch.zeros(rows, H, dtype=torch.float64)
    x[pat == 0, 0] = 1.0
    x[pat == 1, I - 1] = 1.0
    h[pat == 2, 0] = 1.0
    h[pat == 3, H - 1] = 1.0

    def pow2(rows_, cols):
        r, c = torch.arange(rows_).unsqueeze(1), torch.arange(cols).unsqueeze(0)
        return torch.pow(2.0, -((3 * c + r) % 7).double()) * (1 - 2 * ((r + c) % 2)).double()
    w = [pow2(3 * H, I), pow2(3 * H, H), torch.zeros(3 * H, dtype=torch.float64), torch.zeros(3 * H, dtype=torch.float64)]
    h_ref, pre = _ref_cell(x, h, None, *w)
    want = {0: w[0][:, 0], 1: w[0][:, I - 1], 2: w[1][:, 0], 3: w[1][:, H - 1]}
    for p_, col in want.items():                                                # the reference itself: a single weight per pre-activation
        m = int((pat == p_).nonzero()[0])
        side = (col[:H], col[H:2 * H], col[2 * H:])
        zero = torch.zeros(H, dtype=torch.float64)
        assert torch.equal(pre[0][m], side[0]) and torch.equal(pre[1][m], side[1])
        assert torch.equal(pre[2][m], side[2] if p_ < 2 else zero) and torch.equal(pre[3][m], zero if p_ < 2 else side[2])
    xd, hd = _f32(x, h)
    ho, gates = _raw_cell(xd, I, hd, None, _f32(*w), rows, I, H)
    assert torch.equal(gates[:, 3 * H:].cpu().double(), pre[3])                 # hn: exact
    errs = _errs(ho, gates, h_ref, pre)
    print(f"gru k pin {(rows, I, H)} [{precision}]: r {errs[1]:.3g}, z {errs[2]:.3g}, n {errs[3]:.3g} (allowed {4 * POINTWISE_FP32:.3g})")
    assert max(errs[1:4]) <= 4 * POINTWISE_FP32
    assert _consistent(ho, gates, hd, None)


@pytest.mark.parametrize("M,I,H", SHAPES)
def test_one_step_backward_matches_float64_autograd(M, I, H, precision):
    """dx, dh_prev, dW_ih, dW_hh, db_ih, db_hh of sum(gh * h'), rows with and without reset."""
    _need_gpu()
    from shifu_amd.rl.recurrent import gru_cell
    w = [t.requires_grad_(True) for t in _weights(I, H, seed=M + H + 1)]
    x, h, reset = _inputs(M, I, H, seed=M + 1, with_reset=M > 1)
    g = torch.Generator().manual_seed(9)
    gh = torch.randn(M, H, generator=g, dtype=torch.float64)
    xs = [t.requires_grad_(True) for t in (x, h)]
    h_ref, _ = _ref_cell(*xs, reset, *w)
    (gh * h_ref).sum().backward()
    wd = [t.requires_grad_(True) for t in _f32(*w)]
    xd = [t.requires_grad_(True) for t in _f32(*xs)]
    hd = gru_cell(*xd, None if reset is None else reset.to(DEV), *wd)
    (gh.to(DEV, torch.float32) * hd).sum().backward()
    tmax = TOL[precision][0]
    names = ["dx", "dh_prev", "dW_ih", "dW_hh", "db_ih", "db_hh"]
    for name, got, ref in zip(names, xd + wd, xs + w):
        scale = float(ref.grad.abs().max()) + 1e-12
        err = float((got.grad.cpu().double() - ref.grad).abs().max())
        print(f"gru backward {(M, I, H)} [{precision}] {name}: err {err:.3g} = {err / scale:.3g} of scale (ceiling {4 * tmax:.3g})")
        assert err <= 4 * tmax * scale, name
    if reset is not None:
        assert (xd[1].grad[reset.bool().to(DEV)] == 0).all()


@pytest.mark.parametrize("layers", [1, 2])
def test_sequence_with_resets_matches_float64(layers, precision):
    """Memory.forward_sequence on the kernel (T = 4, resets inside, a carried state) against the stock module in float64: outputs
    and parameter gradients.  GEMMs chained on the longest path: T + layers - 1 cell GEMMs forward (P); for a gradient the same P
    forward, then P - 1 input-gradient GEMMs back through time / layers and the weight-gradient GEMM: 2 P."""
    _need_gpu()
    from shifu_amd.rl import Memory
    T, n, I, H = 4, 33, 19, 40
    torch.manual_seed(4)
    ref = Memory(I, type="gru", num_layers=layers, hidden_size=H).double()
    mem = Memory(I, type="gru", num_layers=layers, hidden_size=H, fused=True)
    mem.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    mem = mem.to(DEV)
    assert mem.fused and mem._use_kernel(torch.zeros(1, I, device=DEV))
    obs = torch.randn(T, n, I, dtype=torch.float64)
    dones = torch.rand(T, n) < 0.3
    dones[0, 0] = dones[T - 1, 1] = True
    hid = torch.randn(layers, n, H, dtype=torch.float64) * 0.5
    wgt = torch.randn(T * n, H, dtype=torch.float64)
    out_ref = ref.forward_sequence(obs, dones, hid)
    (wgt * out_ref).sum().backward()
    out = mem.forward_sequence(obs.to(DEV, torch.float32), dones.to(DEV), hid.to(DEV, torch.float32))
    (wgt.to(DEV, torch.float32) * out).sum().backward()
    P, tmax = T + layers - 1, TOL[precision][0]
    scale = float(out_ref.detach().abs().max())
    err = float((out.detach().cpu().double() - out_ref.detach()).abs().max())
    print(f"gru sequence L={layers} [{precision}] outputs: err {err / scale:.3g} of scale (ceiling {P * tmax:.3g})")
    assert err <= P * tmax * scale
    for (name, p), q in zip(mem.rnn.named_parameters(), ref.rnn.parameters()):
        scale = float(q.grad.abs().max()) + 1e-12
        err = float((p.grad.cpu().double() - q.grad).abs().max())
        print(f"gru sequence L={layers} [{precision}] {name}: err {err / scale:.3g} of scale (ceiling {2 * P * tmax:.3g})")
        assert err <= 2 * P * tmax * scale, name


def test_rows_are_independent_bitwise():
    """Permuted rows and a subset of rows equal the same rows of the full call bit for bit; a NaN in one row of x stays there."""
    _need_gpu()
    M, I, H = 70, 19, 96
    w = _f32(*_weights(I, H, seed=1))
    x, h, reset = _f32(*_inputs(M, I, H, seed=2, with_reset=True))
    ho, go = _raw_cell(x, I, h, reset, w, M, I, H)
    perm = torch.randperm(M, generator=torch.Generator().manual_seed(0)).to(DEV)
    hp, gp = _raw_cell(x[perm].contiguous(), I, h[perm].contiguous(), reset[perm].contiguous(), w, M, I, H)
    assert torch.equal(hp, ho[perm]) and torch.equal(gp, go[perm])
    sub = perm[:33].sort().values
    hs, gs = _raw_cell(x[sub].contiguous(), I, h[sub].contiguous(), reset[sub].contiguous(), w, 33, I, H)
    assert torch.equal(hs, ho[sub]) and torch.equal(gs, go[sub])
    xn = x.clone()
    xn[41, 7] = float("nan")
    hn, _ = _raw_cell(xn, I, h, reset, w, M, I, H, want_gates=False)
    rest = torch.arange(M, device=DEV) != 41
    assert torch.isnan(hn[41]).all()
    assert torch.equal(hn[rest], ho[rest])


def test_host_entry_refuses_aliasing_misalignment_and_a_short_stride():
    """The refusal paths only: nothing is launched, every message comes from shf_mlp_last_error."""
    _need_gpu()
    from shifu_amd._lib import lib
    L = lib()
    M, I, H = 8, 5, 32
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    nb = C.c_int64()
    assert L.shf_gru_pack_bytes(I, H, C.byref(nb)) == 0
    pack = torch.zeros(nb.value + 16, device=DEV, dtype=torch.uint8)
    x, h = torch.zeros(M, I, device=DEV), torch.zeros(M, H, device=DEV)
    out = torch.full((M, H), 7.0, device=DEV)
    fwd = lambda x_=p(x), ldx=I, h_out=p(out), pk=p(pack): L.shf_gru_cell_forward(x_, ldx, p(h), None, pk, None, None, h_out, None, M, I, H, None)
    assert fwd(h_out=p(h)) != 0 and "overlap" in L.shf_mlp_last_error().decode()
    assert fwd(h_out=p(h, 4 * H)) != 0 and "overlap" in L.shf_mlp_last_error().decode()
    assert fwd(pk=p(pack, 4)) != 0 and "aligned" in L.shf_mlp_last_error().decode()
    assert fwd(ldx=I - 1) != 0 and "ldx" in L.shf_mlp_last_error().decode()
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (h == 0).all()


def _policy_pair(layers=1):
    from shifu_amd.rl import ActorCriticRecurrent
    torch.manual_seed(6)
    kw = dict(actor_hidden_dims=[64, 32], critic_hidden_dims=[64, 32], rnn_type="gru", rnn_hidden_size=96, rnn_num_layers=layers,
              mlp_backend="mfma")
    fused = ActorCriticRecurrent(19, 23, 5, rnn_fused=True, **kw).to(DEV)
    stock = ActorCriticRecurrent(19, 23, 5, rnn_fused=False, **kw)
    stock.load_state_dict(fused.state_dict())
    assert fused.memory_a.fused and fused.memory_c.fused and not stock.memory_a.fused
    assert ActorCriticRecurrent(19, 23, 5, **kw).memory_a.fused is False        # the GRU's default stays the stock module
    return fused, stock.to(DEV)


def test_policy_on_the_fused_path_matches_the_stock_path():
    """act_inference step by step (two steps, a reset between them), then the sequence entry with a loss gradient: the kernel
    path against torch.nn.GRU with the same weights, within the chained-GEMM ceiling (cells + MLP layers; for a parameter
    gradient the forward chain, the input-gradient GEMMs back through it and the weight-gradient GEMM)."""
    _need_gpu()
    from shifu_amd.rl.mfma_linear import refresh_packs
    layers = 2
    fused, stock = _policy_pair(layers)
    tmax, n = TOL["bf16x3"][0], 50

    def close(got, ref, gemms, what):
        err, scale = float((got - ref).abs().max()), float(ref.abs().max()) + 1e-12
        print(f"gru policy {what}: err {err / scale:.3g} of scale (ceiling {gemms * tmax:.3g})")
        assert err <= gemms * tmax * scale, what

    with torch.no_grad():
        refresh_packs(fused)
        assert fused.memory_a._pack_valid and fused.memory_c._pack_valid
        for step in range(2):
            obs, cobs = torch.randn(n, 19, device=DEV), torch.randn(n, 23, device=DEV)
            close(fused.act_inference(obs), stock.act_inference(obs), (step + layers) + 3, f"act_inference step {step}")
            close(fused.evaluate(cobs), stock.evaluate(cobs), (step + layers) + 3, f"evaluate step {step}")
            close(fused.get_hidden_states()[0], stock.get_hidden_states()[0], step + layers, f"hidden state step {step}")
            dones = torch.rand(n, device=DEV) < 0.3
            fused.reset(dones)
            stock.reset(dones)
            assert (fused.get_hidden_states()[0][:, dones] == 0).all()
    T = 4
    obs, cobs = torch.randn(T, n, 19, device=DEV), torch.randn(T, n, 23, device=DEV)
    dones = torch.rand(T, n, device=DEV) < 0.3
    hid = tuple(h.clone() for h in stock.get_hidden_states())
    wa, wc = torch.randn(T * n, 96, device=DEV), torch.randn(T * n, 96, device=DEV)
    feats = []
    for ac in (fused, stock):
        fa, fc = ac.sequence_features(obs, cobs, dones, hid)
        ((wa * fa).sum() + (wc * fc).sum()).backward()
        feats.append((fa.detach(), fc.detach()))
    P = T + layers - 1
    close(feats[0][0], feats[1][0], P, "sequence features (actor)")
    close(feats[0][1], feats[1][1], P, "sequence features (critic)")
    for mem in ("memory_a", "memory_c"):
        for (name, p), q in zip(getattr(fused, mem).rnn.named_parameters(), getattr(stock, mem).rnn.parameters()):
            close(p.grad, q.grad, 2 * P, f"{mem}.{name} gradient")


def _a1_runner(graph, envs=8, steps=4):
    from examples.a1_conditional.task_config import A1PPOConfig
    from shifu_amd.gym.a1_fused import FusedA1Env
    from shifu_amd.rl import OnPolicyRunner
    from shifu_amd.runner.utils import class_to_dict
    cfg = class_to_dict(A1PPOConfig())
    cfg["runner"].update({"policy_class_name": "ActorCriticRecurrent", "num_steps_per_env": steps, "graph_rollout": graph})
    cfg["policy"].update({"mlp_backend": "mfma", "rnn_type": "gru", "rnn_fused": True, "rnn_hidden_size": 128, "rnn_num_layers": 1})
    torch.manual_seed(0)
    env = FusedA1Env(num_envs=envs, group=32, seed=5)
    return OnPolicyRunner(env, cfg, log_dir=None, device=DEV), env


def test_captured_rollout_equals_the_eager_rollout_bitwise():
    """graph_rollout with the fused GRU, 8 envs x 4 steps: the second iteration's rollout is captured and replayed; storage
    contents and hidden states equal the eager runner's bit for bit (the state buffers keep their addresses)."""
    _need_gpu()
    got = []
    for graph in (False, True):
        runner, env = _a1_runner(graph)
        ac = runner.alg.actor_critic
        assert ac.memory_a.fused and ac.memory_a.kind == "gru"
        runner.learn(2, init_at_random_ep_len=True)
        torch.cuda.synchronize()
        st = runner.alg.storage
        got.append([st.observations, st.actions, st.rewards, st.dones, st.values, st.actions_log_prob, st.mu, st.sigma]
                   + list(st.saved_hidden_states_a + st.saved_hidden_states_c) + list(ac.get_hidden_states()))
    names = ["observations", "actions", "rewards", "dones", "values", "log_prob", "mu", "sigma"] + ["saved hidden"] * 2 + ["hidden"] * 2
    assert len(got[0]) == len(names)
    for name, a, b in zip(names, *got):
        assert torch.equal(a, b), name
    assert float(got[0][-1].abs().max()) > 0
