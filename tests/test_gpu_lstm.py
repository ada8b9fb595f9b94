"""The fused LSTM cell step (shifu_amd/csrc/shf_lstm.hip) and the recurrent policy on it, against float64 torch on the CPU.

Forward bound (derived).  The GEMM's pre-activations carry an error e = tmax * max|pre| (tmax: TOL of
tests/test_gpu_mlp.py for the operand precision; the scale from the float64 reference).  With sigma' <= 1/4, tanh' <= 1,
|gates| <= 1:   |dc'| <= (|c|/4 + 1/4 + 1) e = (1.25 + max|c_prev|/4) e,   |dh'| <= e/4 + |dc'| = (1.5 + max|c_prev|/4) e.
The fp32 pointwise arithmetic adds an absolute term: the same formulas evaluated by torch in fp32 on the GPU from the
float64 pre-activations differ from float64 by at most POINTWISE_FP32 on these inputs (measured, printed by the test);
four times that is allowed for another exp form.

Backward ceilings: one step 3 x TOL of each tensor's scale (the forward gates, the derivative evaluated at them, the
gradient GEMM); a sequence: the number of GEMMs chained on the longest path x TOL."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from tests.test_gpu_mlp import TOL      # noqa: E402

DEV = "cuda:0"
SHAPES = [(1, 5, 32), (33, 5, 40), (70, 19, 96), (64, 259, 512)]
# max |fp32 torch pointwise - float64| over the inputs of test_forward_matches_float64, measured on an MI355X: 1.51e-7 (c'), 9.75e-8 (h')
POINTWISE_FP32 = 1.51e-7


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
    u = lambda *s: (torch.rand(*s, generator=g, dtype=torch.float64) * 2 - 1) * k      # nn.LSTM's initialisation
    return u(4 * H, I), u(4 * H, H), u(4 * H), u(4 * H)


def _inputs(M, I, H, seed, with_reset):
    g = torch.Generator().manual_seed(seed + 100)
    x = torch.randn(M, I, generator=g, dtype=torch.float64) * 1.5
    h = torch.randn(M, H, generator=g, dtype=torch.float64) * 0.5
    c = torch.rand(M, H, generator=g, dtype=torch.float64) * 2 - 1                      # |c_prev| <= 1
    reset = None
    if with_reset:
        reset = (torch.rand(M, generator=g) < 0.4).to(torch.uint8)
        reset[0] = 1
    return x, h, c, reset


def _ref_cell(x, h, c, reset, w_ih, w_hh, b_ih, b_hh):
    """float64: (h', c', pre-activations) with the reset by multiplication."""
    keep = 1.0 if reset is None else (1.0 - reset.to(x.dtype)).unsqueeze(1)
    pre = x @ w_ih.t() + b_ih + (h * keep) @ w_hh.t() + b_hh
    i, f, g, o = pre.chunk(4, dim=1)
    cn = torch.sigmoid(f) * (c * keep) + torch.sigmoid(i) * torch.tanh(g)
    return torch.sigmoid(o) * torch.tanh(cn), cn, pre


def _f32(*ts):
    return [None if t is None else (t.to(DEV) if t.dtype == torch.uint8 else t.to(DEV, torch.float32)) for t in ts]


def _raw_cell(x, ldx, h, c, reset, w, M, I, H, want_gates=True):
    """The C entries directly: pack, then one cell step; x is read through the row stride ldx."""
    from shifu_amd._lib import lib
    L = lib()
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    nb = C.c_int64()
    assert L.shf_lstm_pack_bytes(I, H, C.byref(nb)) == 0
    pack = torch.empty(nb.value, device=DEV, dtype=torch.uint8)
    assert L.shf_lstm_pack_weights(p(w[0]), p(w[1]), p(pack), I, H, st) == 0, L.shf_mlp_last_error()
    ho, co = torch.full((M, H), 7.0, device=DEV), torch.full((M, H), -7.0, device=DEV)
    gates = torch.full((M, 4 * H), 9.0, device=DEV) if want_gates else None
    rc = L.shf_lstm_cell_forward(p(x), ldx, p(h), p(c), p(reset), p(pack), p(w[2]), p(w[3]), p(ho), p(co), p(gates), M, I, H, st)
    assert rc == 0, L.shf_mlp_last_error()
    return ho, co, gates


@pytest.mark.parametrize("M,I,H", [(33, 5, 40), (70, 19, 96)])
def test_saturated_gates_pin_gate_order_and_unit_index(M, I, H, precision):
    """All weights zero except five entries that drive ONE gate of ONE unit to +-32 (sigma = 1, tanh = -1 exactly in fp32; every
    other gate is sigma(0) = 0.5 / tanh(0) = 0), so c' is exact: a gate tile, a unit or a k index in the wrong place cannot pass.
      unit a: f = 1 (through x)          -> c' = c            unit b: g = -1 (through h_prev)  -> c' = c/2 - 1/2
      unit d: i = 1 and g = -1           -> c' = c/2 - 1      unit e: o = 1                   -> c' = c/2, h' doubled
    The saturating x / h entries are set in every third row only, the cell state is a small integer per (row, unit)."""
    _need_gpu()
    a, b, d, e = 3, 33, H - 2, H - 1
    w_ih, w_hh = torch.zeros(4 * H, I), torch.zeros(4 * H, H)
    bias = torch.zeros(4 * H)
    w_ih[1 * H + a, 2] = 8.0                       # f of unit a  <- x[:, 2]
    w_hh[2 * H + b, 5] = -8.0                      # g of unit b  <- h_prev[:, 5]
    w_ih[0 * H + d, I - 1] = 8.0                   # i of unit d  <- x[:, I - 1]
    w_hh[2 * H + d, H - 1] = -8.0                  # g of unit d  <- h_prev[:, H - 1]
    w_hh[3 * H + e, 0] = 8.0                       # o of unit e  <- h_prev[:, 0]
    hot = (torch.arange(M) % 3 == 0).float()
    ldx = I + 3                                    # x is a column block of a wider matrix
    xw = torch.full((M, ldx), 77.0)
    xw[:, :I] = 0.0
    xw[:, 2] = 4.0 * hot
    xw[:, I - 1] = 4.0 * hot
    h = torch.zeros(M, H)
    h[:, 5] = h[:, H - 1] = h[:, 0] = 4.0 * hot
    c = ((torch.arange(M).unsqueeze(1) * 3 + torch.arange(H).unsqueeze(0)) % 7 - 3).float()
    half = torch.full((M, H), 0.5)
    gi, gf, gg, go = half.clone(), half.clone(), torch.zeros(M, H), half.clone()
    on = hot.bool()
    gf[on, a] = 1.0
    gg[on, b] = -1.0
    gi[on, d] = 1.0
    gg[on, d] = -1.0
    go[on, e] = 1.0
    c_want = gf * c + gi * gg                      # exact in fp32: halves of small integers
    ho, co, gates = _raw_cell(*_f32(xw), ldx, *_f32(h, c), None, _f32(w_ih, w_hh, bias, bias), M, I, H)
    assert torch.equal(co.cpu(), c_want)
    assert torch.equal(gates.cpu(), torch.cat([gi, gf, gg, go], dim=1))
    torch.testing.assert_close(ho.cpu(), go * torch.tanh(c_want), rtol=0, atol=1e-6)
    assert float((ho.cpu()[on, e] - 2 * (0.5 * torch.tanh(c_want))[on, e]).abs().max()) <= 1e-6


@pytest.mark.parametrize("with_reset", [False, True])
@pytest.mark.parametrize("M,I,H", SHAPES)
def test_forward_matches_float64(M, I, H, with_reset, precision):
    _need_gpu()
    w = _weights(I, H, seed=M + H)
    x, h, c, reset = _inputs(M, I, H, seed=M, with_reset=with_reset)
    h_ref, c_ref, pre = _ref_cell(x, h, c, reset, *w)
    ho, co, gates = _raw_cell(*_f32(x), I, *_f32(h, c, reset), _f32(*w), M, I, H)
    # the absolute term: torch's fp32 pointwise formulas on the GPU from the same pre-activations, against float64
    p32 = pre.to(DEV, torch.float32)
    keep = 1.0 if reset is None else (1.0 - reset.to(DEV, torch.float32)).unsqueeze(1)
    i_, f_, g_, o_ = p32.chunk(4, dim=1)
    c32 = torch.sigmoid(f_) * (c.to(DEV, torch.float32) * keep) + torch.sigmoid(i_) * torch.tanh(g_)
    h32 = torch.sigmoid(o_) * torch.tanh(c32)
    pw_c, pw_h = float((c32.cpu().double() - c_ref).abs().max()), float((h32.cpu().double() - h_ref).abs().max())
    e = TOL[precision][0] * float(pre.abs().max())
    cmax = float(c.abs().max())
    bound_c, bound_h = (1.25 + cmax / 4) * e + 4 * POINTWISE_FP32, (1.5 + cmax / 4) * e + 4 * POINTWISE_FP32
    err_c, err_h = float((co.cpu().double() - c_ref).abs().max()), float((ho.cpu().double() - h_ref).abs().max())
    print(f"lstm forward {(M, I, H)} reset={with_reset} [{precision}]: err c' {err_c:.3g} (bound {bound_c:.3g}), h' {err_h:.3g} "
          f"(bound {bound_h:.3g}); torch fp32 pointwise vs float64: c' {pw_c:.3g}, h' {pw_h:.3g}; max|pre| {float(pre.abs().max()):.3g}")
    assert err_c <= bound_c and err_h <= bound_h
    # the kept gates are the activated ones, in torch's order
    i, f, g, o = pre.chunk(4, dim=1)
    g_ref = torch.cat([torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)], dim=1)
    assert float((gates.cpu().double() - g_ref).abs().max()) <= e + 4 * POINTWISE_FP32
    if with_reset:      # a finished row does not see its h_prev / c_prev at all
        h2, c2 = h.clone(), c.clone()
        h2[reset.bool()] = 123.0
        c2[reset.bool()] = -55.0
        ho2, co2, _ = _raw_cell(*_f32(x), I, *_f32(h2, c2, reset), _f32(*w), M, I, H)
        assert torch.equal(ho2, ho) and torch.equal(co2, co)


@pytest.mark.parametrize("M,I,H", SHAPES)
def test_one_step_backward_matches_float64_autograd(M, I, H, precision):
    """dx, dh_prev, dc_prev, dW_ih, dW_hh, db_ih, db_hh of sum(gh * h') + sum(gc * c'), rows with and without reset."""
    _need_gpu()
    from shifu_amd.rl.recurrent import lstm_cell
    w = [t.requires_grad_(True) for t in _weights(I, H, seed=M + H + 1)]
    x, h, c, reset = _inputs(M, I, H, seed=M + 1, with_reset=M > 1)
    g = torch.Generator().manual_seed(9)
    gh, gc = torch.randn(M, H, generator=g, dtype=torch.float64), torch.randn(M, H, generator=g, dtype=torch.float64)
    xs = [t.requires_grad_(True) for t in (x, h, c)]
    h_ref, c_ref, _ = _ref_cell(*xs, reset, *w)
    ((gh * h_ref).sum() + (gc * c_ref).sum()).backward()
    wd = [t.requires_grad_(True) for t in _f32(*[t.detach() for t in w])]
    xd = [t.requires_grad_(True) for t in _f32(*[t.detach() for t in xs])]
    hd, cd = lstm_cell(*xd, None if reset is None else reset.to(DEV), *wd)
    ((gh.to(DEV, torch.float32) * hd).sum() + (gc.to(DEV, torch.float32) * cd).sum()).backward()
    tmax = TOL[precision][0]
    names = ["dx", "dh_prev", "dc_prev", "dW_ih", "dW_hh", "db_ih", "db_hh"]
    for name, got, ref in zip(names, xd + wd, xs + w):
        scale = float(ref.grad.abs().max()) + 1e-12
        err = float((got.grad.cpu().double() - ref.grad).abs().max())
        print(f"lstm backward {(M, I, H)} [{precision}] {name}: err {err:.3g} = {err / scale:.3g} of scale (ceiling {3 * tmax:.3g})")
        assert err <= 3 * tmax * scale, name
    if reset is not None:
        r = reset.bool()
        assert (xd[1].grad[r.to(DEV)] == 0).all() and (xd[2].grad[r.to(DEV)] == 0).all()


@pytest.mark.parametrize("layers", [1, 2])
def test_sequence_with_resets_matches_float64(layers, precision):
    """Memory.forward_sequence on the kernel (T = 4, resets inside) against the stock module in float64: outputs and parameter
    gradients.  GEMMs chained on the longest path: T + layers - 1 cell GEMMs forward (P); for a gradient the same P forward, then
    P - 1 input-gradient GEMMs back through time / layers and the weight-gradient GEMM: 2 P."""
    _need_gpu()
    from shifu_amd.rl import Memory
    T, n, I, H = 4, 33, 19, 40
    torch.manual_seed(4)
    ref = Memory(I, num_layers=layers, hidden_size=H).double()
    mem = Memory(I, num_layers=layers, hidden_size=H, fused=True)
    mem.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    mem = mem.to(DEV)
    obs = torch.randn(T, n, I, dtype=torch.float64)
    dones = torch.rand(T, n) < 0.3
    dones[0, 0] = dones[T - 1, 1] = True
    hid = (torch.randn(layers, n, H, dtype=torch.float64) * 0.5, torch.rand(layers, n, H, dtype=torch.float64) * 2 - 1)
    wgt = torch.randn(T * n, H, dtype=torch.float64)
    out_ref = ref.forward_sequence(obs, dones, hid)
    (wgt * out_ref).sum().backward()
    out = mem.forward_sequence(obs.to(DEV, torch.float32), dones.to(DEV), tuple(t.to(DEV, torch.float32) for t in hid))
    (wgt.to(DEV, torch.float32) * out).sum().backward()
    P, tmax = T + layers - 1, TOL[precision][0]
    scale = float(out_ref.detach().abs().max())
    err = float((out.detach().cpu().double() - out_ref).abs().max())
    print(f"lstm sequence L={layers} [{precision}] outputs: err {err / scale:.3g} of scale (ceiling {P * tmax:.3g})")
    assert err <= P * tmax * scale
    for (name, p), q in zip(mem.rnn.named_parameters(), ref.rnn.parameters()):
        scale = float(q.grad.abs().max()) + 1e-12
        err = float((p.grad.cpu().double() - q.grad).abs().max())
        print(f"lstm sequence L={layers} [{precision}] {name}: err {err / scale:.3g} of scale (ceiling {2 * P * tmax:.3g})")
        assert err <= 2 * P * tmax * scale, name


def test_rows_are_independent_bitwise():
    """Permuted rows and a subset of rows equal the same rows of the full call bit for bit; a NaN in one row of x stays there."""
    _need_gpu()
    M, I, H = 70, 19, 96
    w = _f32(*_weights(I, H, seed=1))
    x, h, c, reset = _f32(*_inputs(M, I, H, seed=2, with_reset=True))
    ho, co, _ = _raw_cell(x, I, h, c, reset, w, M, I, H, want_gates=False)
    perm = torch.randperm(M, generator=torch.Generator().manual_seed(0)).to(DEV)
    hp, cp, _ = _raw_cell(x[perm].contiguous(), I, h[perm].contiguous(), c[perm].contiguous(), reset[perm].contiguous(), w, M, I, H, False)
    assert torch.equal(hp, ho[perm]) and torch.equal(cp, co[perm])
    sub = perm[:33].sort().values
    hs, cs, _ = _raw_cell(x[sub].contiguous(), I, h[sub].contiguous(), c[sub].contiguous(), reset[sub].contiguous(), w, 33, I, H, False)
    assert torch.equal(hs, ho[sub]) and torch.equal(cs, co[sub])
    xn = x.clone()
    xn[41, 7] = float("nan")
    hn, cn, _ = _raw_cell(xn, I, h, c, reset, w, M, I, H, want_gates=False)
    rest = torch.arange(M, device=DEV) != 41
    assert torch.isnan(hn[41]).all() and torch.isnan(cn[41]).all()
    assert torch.equal(hn[rest], ho[rest]) and torch.equal(cn[rest], co[rest])


def _policy_pair(layers=1):
    from shifu_amd.rl import ActorCriticRecurrent
    torch.manual_seed(6)
    kw = dict(actor_hidden_dims=[64, 32], critic_hidden_dims=[64, 32], rnn_hidden_size=96, rnn_num_layers=layers)
    fused = ActorCriticRecurrent(19, 23, 5, mlp_backend="mfma", **kw).to(DEV)
    stock = ActorCriticRecurrent(19, 23, 5, mlp_backend="torch", **kw)
    stock.load_state_dict(fused.state_dict())
    assert fused.memory_a.fused and not stock.memory_a.fused
    return fused, stock.to(DEV)


def test_policy_on_the_fused_path_matches_the_stock_path():
    """act / evaluate step by step (two steps, a reset between them) and the sequence entry: the kernel path against
    torch.nn.LSTM + fp32 library GEMMs with the same weights, within the chained-GEMM ceiling (cell + MLP layers)."""
    _need_gpu()
    from shifu_amd.rl.mfma_linear import refresh_packs
    fused, stock = _policy_pair(layers=2)
    tmax, n = TOL["bf16x3"][0], 50

    def close(got, ref, gemms, what):
        err, scale = float((got - ref).abs().max()), float(ref.abs().max())
        print(f"policy {what}: err {err / scale:.3g} of scale (ceiling {gemms * tmax:.3g})")
        assert err <= gemms * tmax * scale, what

    with torch.no_grad():
        refresh_packs(fused)
        assert fused.memory_a._pack_valid and fused.memory_c._pack_valid
        for step in range(2):
            obs, cobs = torch.randn(n, 19, device=DEV), torch.randn(n, 23, device=DEV)
            for ac in (fused, stock):
                ac.act(obs)
            close(fused.action_mean, stock.action_mean, (step + 2) + 3, f"act step {step}")           # cells chained so far + three MLP layers
            close(fused.evaluate(cobs), stock.evaluate(cobs), (step + 2) + 3, f"evaluate step {step}")
            for a, b in zip(fused.get_hidden_states()[0], stock.get_hidden_states()[0]):
                close(a, b, step + 2, f"hidden state step {step}")
            dones = torch.rand(n, device=DEV) < 0.3
            fused.reset(dones)
            stock.reset(dones)
            assert (fused.get_hidden_states()[0][0][:, dones] == 0).all()
    T = 4
    obs, cobs = torch.randn(T, n, 19, device=DEV), torch.randn(T, n, 23, device=DEV)
    dones = torch.rand(T, n, device=DEV) < 0.3
    hid = stock.get_hidden_states()
    fa, fc = fused.sequence_features(obs, cobs, dones, hid)
    sa, sc = stock.sequence_features(obs, cobs, dones, hid)
    close(fa.detach(), sa.detach(), T + 1, "sequence features (actor)")
    close(fc.detach(), sc.detach(), T + 1, "sequence features (critic)")


def _a1_runner(graph, tmp=None, envs=64, steps=4, **env_kw):
    from examples.a1_conditional.task_config import A1PPOConfig
    from shifu_amd.gym.a1_fused import FusedA1Env
    from shifu_amd.rl import OnPolicyRunner
    from shifu_amd.runner.utils import class_to_dict
    cfg = class_to_dict(A1PPOConfig())
    cfg["runner"].update({"policy_class_name": "ActorCriticRecurrent", "num_steps_per_env": steps, "graph_rollout": graph})
    cfg["policy"].update({"mlp_backend": "mfma", "rnn_type": "lstm", "rnn_hidden_size": 128, "rnn_num_layers": 1})
    torch.manual_seed(0)
    env = FusedA1Env(num_envs=envs, group=32, seed=5, **env_kw)
    return OnPolicyRunner(env, cfg, log_dir=tmp, device=DEV), env


def test_captured_rollout_equals_the_eager_rollout_bitwise():
    """graph_rollout with a recurrent policy: the second iteration's rollout is captured and replayed; storage contents and
    hidden states equal the eager runner's bit for bit (the state buffers keep their addresses, reset() multiplies in place)."""
    _need_gpu()
    got = []
    for graph in (False, True):
        runner, env = _a1_runner(graph)
        assert runner.alg.actor_critic.memory_a.fused
        runner.learn(2, init_at_random_ep_len=True)
        torch.cuda.synchronize()
        st, ac = runner.alg.storage, runner.alg.actor_critic
        hs = [h for pair in ac.get_hidden_states() for h in pair]
        got.append([st.observations, st.actions, st.rewards, st.dones, st.values, st.actions_log_prob, st.mu, st.sigma]
                   + list(st.saved_hidden_states_a + st.saved_hidden_states_c) + hs)
    names = ["observations", "actions", "rewards", "dones", "values", "log_prob", "mu", "sigma"] + ["saved hidden"] * 4 + ["hidden"] * 4
    for name, a, b in zip(names, *got):
        assert torch.equal(a, b), name
    assert float(got[0][-1].abs().max()) > 0


def test_recurrent_training_runs_on_the_fused_env(tmp_path):
    _need_gpu()
    runner, env = _a1_runner(False, str(tmp_path), steps=24, episode_length_s=0.2)
    ac = runner.alg.actor_critic
    before = [p.detach().clone() for p in ac.parameters()]
    runner.learn(3, init_at_random_ep_len=True)
    assert len(runner.history) == 3
    for h in runner.history:
        assert np.isfinite(h["value_loss"]) and np.isfinite(h["surrogate_loss"])
    for (name, p), q in zip(ac.named_parameters(), before):
        assert torch.isfinite(p).all() and not torch.equal(p.detach(), q), name
    done = runner.alg.storage.dones[-1, :, 0].bool()
    assert int(done.sum()) > 0, "the check below needs envs that finished in the last step"
    for h in [h for pair in ac.get_hidden_states() for h in pair]:
        assert (h[:, done] == 0).all() and float(h[:, ~done].abs().max()) > 0
    other, _ = _a1_runner(False)
    other.load(str(tmp_path / "model_3.pt"))
    obs = env.get_observations().clone()
    pa, pb = runner.get_inference_policy(), other.get_inference_policy()
    ac.reset()
    other.alg.actor_critic.reset()
    with torch.no_grad():
        for _ in range(2):                   # the second call runs from the carried state
            assert torch.equal(pa(obs), pb(obs))
