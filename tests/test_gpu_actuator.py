"""The actuator models on the GPU (csrc/shf_actuator.hip: shf_actuator_step) and what stands on them (glue.actuator_step,
units.actuators.Actuator, Robot.set_actuator / apply_actuator_targets).

Kernel against twin.  tests/actuator_ref.py `step32` is the kernel's header in NumPy float32, operation by operation; 20
consecutive calls with the state carried on both sides, fresh seeded targets and dof states per call, per-env delays, strengths
and gains, resets on calls 5 and 11.  Efforts, applied targets and the three histories must be bit-equal at every call for PD, the
DC motor and the networks with softsign and relu.  tanh and elu go through the maths library: there the states are still
bit-equal and the efforts are held against `step64`; WORST below is the largest |kernel - step64| in N m over every shape and
call measured on an MI355X, asserted at four times that (another exp form may differ by a few ulp) and never above the
worst-case forward error of the float32 network from its actual weights (`bound`).  Measured: tanh 7.191e-6 N m, elu 1.053e-5
N m (both on 8-64-64-1 at 257 x 12, torques up to 33.5 N m, where one float32 ulp is 3.8e-6); softsign, which is bit-equal to
step32, stands 5.43e-6 N m from step64 on the same cases.
"""
import ctypes

import numpy as np
import pytest

from tests import actuator_ref as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CALLS = 20
SHAPES = [(1, 12), (65, 5), (257, 12)]        # 65 x 5 = 325 rows: a partial last wavefront, and an env's dofs straddle wavefronts
SAT, VLIM, LIM = 33.5, 21.0, 33.5
WORST = {"tanh": 7.191e-6, "elu": 1.053e-5}   # MI355X, see the docstring
NETS = {"softsign-6-32-32-32-1": ([6, 32, 32, 32, 1], "softsign"), "relu-6-32-32-32-1": ([6, 32, 32, 32, 1], "relu"),
        "softsign-2-8-1": ([2, 8, 1], "softsign"), "relu-8-64-64-1": ([8, 64, 64, 1], "relu"), "softsign-8-64-64-1": ([8, 64, 64, 1], "softsign"),
        "softsign-6-33-5-1": ([6, 33, 5, 1], "softsign"), "relu-6-33-5-1": ([6, 33, 5, 1], "relu"), "softsign-6-1": ([6, 1], "softsign")}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible (these tests never fall back to CPU)")


def _net(widths, activation, seed=3):
    T = widths[0] // 2
    return R.make_net(widths, activation, taps=tuple(range(T)) if T != 3 else (0, 1, 2), err_scale=2.0, vel_scale=0.1, out_scale=20.0, seed=seed)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _case(n, nd, net, dc, L=4, seed=0):
    """The per-case constants on both sides: per-env delays 0..L-1, strengths in [0.8, 1.2], per-env gains, the limits."""
    from shifu_amd.units import ActuatorNet
    rng = np.random.default_rng(seed)
    dev = "cuda:0"
    g = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    c = {"delay": (np.arange(n) % L).astype(np.int32), "strength": rng.uniform(0.8, 1.2, (n, nd)).astype(np.float32),
         "kp": rng.uniform(30, 50, (n, nd)).astype(np.float32), "kd": rng.uniform(0.5, 1.5, (n, nd)).astype(np.float32),
         "effort_limit": np.full(nd, LIM, np.float32)}
    if dc:
        c.update(saturation=np.full(nd, SAT, np.float32), velocity_limit=np.full(nd, VLIM, np.float32))
    gpu = {k: g(v) for k, v in c.items()}
    H = None
    if net is not None:
        H = max(net["taps"]) + 1
        gpu["net"] = ActuatorNet(net["layers"], net["activation"]).bind(dev, net["taps"], net["err_scale"], net["vel_scale"], net["out_scale"])
        gpu["err_hist"], gpu["vel_hist"] = torch.full((n, H, nd), 7.0, device=dev), torch.full((n, H, nd), -7.0, device=dev)
        gpu.pop("kp"), gpu.pop("kd")
    return rng, c, gpu, g, H


def _calls(rng, n, nd, calls=CALLS):
    """Per call: fresh inputs and the reset flags (every env on call 0; about 40 % of them, env 0 among them, on calls 5 and 11)."""
    for k in range(calls):
        X = R.seeded_call(rng, n, nd)
        reset = None
        if k in (0, 5, 11):
            reset = np.ones(n, np.uint8) if k == 0 else (rng.uniform(size=n) < 0.4).astype(np.uint8)
            reset[0] = 1
        yield k, X, reset


def _against_the_twin(n, nd, net, dc, exact):
    """20 calls of the kernel and of step32 (and step64) side by side.  Returns the worst |kernel - step64| and the DC
    branch counts from step64."""
    from shifu_amd import glue
    L = 4
    rng, c, gpu, g, H = _case(n, nd, net, dc, L)
    s32, s64 = R.new_state(n, nd, L, H), R.new_state(n, nd, L, H, np.float64)
    cmd = torch.full((n, L, nd), 3.0, device="cuda:0")             # junk before the first (resetting) call
    applied, out = torch.zeros(n, nd, device="cuda:0"), torch.zeros(n, nd, device="cuda:0")
    worst, counts = 0.0, np.zeros(5)
    for k, X, reset in _calls(rng, n, nd):
        dof = g(np.stack([X["q"], X["qd"]], -1).reshape(n * nd, 2))               # the interleaved dof-state tensor, read in place
        glue.actuator_step(g(X["target"]), dof.view(n, nd, 2), cmd, reset=None if reset is None else g(reset), applied_out=applied,
                           efforts_out=out, **gpu)
        args = dict(c, reset=reset, net=net)
        o32 = R.step32(s32, X["target"], X["q"], X["qd"], **args)
        o64 = R.step64(s64, X["target"], X["q"], X["qd"], **args)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert np.isfinite(got).all()
        assert np.array_equal(_bits(applied.cpu().numpy()), _bits(o32["applied"])), f"applied target, call {k}"
        assert np.array_equal(_bits(cmd.cpu().numpy()), _bits(s32["cmd"])), f"cmd_hist, call {k}"
        if net is not None:
            assert np.array_equal(_bits(gpu["err_hist"].cpu().numpy()), _bits(s32["err"])), f"err_hist, call {k}"
            assert np.array_equal(_bits(gpu["vel_hist"].cpu().numpy()), _bits(s32["vel"])), f"vel_hist, call {k}"
        d = np.abs(got.astype(np.float64) - o64["efforts"])
        worst = max(worst, float(d.max()))
        if exact:
            assert np.array_equal(_bits(got), _bits(o32["efforts"])), f"efforts, call {k}: {int((_bits(got) != _bits(o32['efforts'])).sum())} differ"
        else:
            taps = list(net["taps"])
            x64 = np.concatenate([net["err_scale"] * s64["err"][:, taps], net["vel_scale"] * s64["vel"][:, taps]], 1).transpose(0, 2, 1).reshape(n * nd, -1)
            b = R.bound(net, x64, c["strength"]).reshape(n, nd)
            tol = np.minimum(4.0 * WORST[net["activation"]], b)
            assert (d <= tol).all(), (net["activation"], k, float(d.max()), float(tol.min()))
        if dc:
            pre, hi, lo = o64["pre"], o64["hi"], o64["lo"]
            counts += [(pre > hi).sum(), (pre < lo).sum(), ((pre <= hi) & (pre >= lo)).sum(), (hi < o64["cap"]).sum(), pre.size]
    return worst, counts


# ---------------------------------------------------------------------------------------------------- against the twin --
@pytest.mark.parametrize("dc", [False, True], ids=["pd", "dc-motor"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_pd_and_dc_motor_are_bit_equal_to_the_twin(shape, dc):
    _need_gpu()
    _against_the_twin(*shape, None, dc, True)


@pytest.mark.parametrize("name", list(NETS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_networks_with_softsign_and_relu_are_bit_equal_to_the_twin(shape, name):
    """6-32-32-32-1 (legged_gym's), 2-8-1, 8-64-64-1 (the 64-wide instantiation), 6-33-5-1 (padded in both hidden layers, to 64
    and from 5) and a single layer; every one behind the DC clip."""
    _need_gpu()
    _against_the_twin(*shape, _net(*NETS[name]), True, True)


@pytest.mark.parametrize("activation", ["tanh", "elu"])
def test_tanh_and_elu_states_bit_equal_efforts_within_four_times_the_measured_worst(activation):
    _need_gpu()
    worst = 0.0
    for n, nd in SHAPES:
        for widths in ([6, 32, 32, 32, 1], [8, 64, 64, 1]):
            worst = max(worst, _against_the_twin(n, nd, _net(widths, activation), True, False)[0])
    print(f"[actuator gpu] {activation}: worst |kernel - step64| {worst:.3e} N m (recorded {WORST[activation]:.3e})")


# ------------------------------------------------------------------------------------------------------- the DC branches --
def test_dc_case_takes_every_branch():
    """On the DC case's own inputs (qd ~ N(0, 8^2) rad/s, a pre-clip torque of sigma about 25 N m, sat = lim = 33.5, vlim = 21),
    counted from step64: clipped from above, clipped from below, left alone, and a ceiling below lim (the speed term binds) are
    each at least 5 % of the entries -- while the kernel stays bit-equal to step32 on them."""
    _need_gpu()
    _, counts = _against_the_twin(257, 12, None, True, True)
    shares = counts[:4] / counts[4]
    print("[actuator gpu] DC shares: above %.3f below %.3f alone %.3f speed-limited ceiling %.3f" % tuple(shares))
    assert (shares >= 0.05).all(), shares


# --------------------------------------------------------------------------------------------------- the example's PD --
def test_pd_equals_the_examples_expression_bit_for_bit():
    """PD, delay 0, no strength, effort_limit given, against examples/a1_conditional/a1_conditional.py:56-57 in torch on the GPU."""
    _need_gpu()
    from shifu_amd import glue
    dev = "cuda:0"
    n, nd = 257, 12
    g = torch.Generator(device=dev).manual_seed(4)
    actions = 0.5 * (2 * torch.rand(n, nd, device=dev, generator=g) - 1)
    default_dof_pos = torch.tensor([0.1, 0.8, -1.5, -0.1, 0.8, -1.5, 0.1, 1.0, -1.5, -0.1, 1.0, -1.5], device=dev)
    dof_state = torch.stack([default_dof_pos + 0.3 * torch.randn(n, nd, device=dev, generator=g), 8.0 * torch.randn(n, nd, device=dev, generator=g)], -1)
    dof_pos, dof_vel = dof_state[..., 0], dof_state[..., 1]
    p_gains, d_gains = torch.full((nd,), 20.0, device=dev), torch.full((nd,), 0.5, device=dev)
    lim = torch.tensor([20.0, 55.0, 55.0] * 4, device=dev) * 0.3                     # low enough to bind on many entries
    want = torch.clip(p_gains * (actions + default_dof_pos - dof_pos) - d_gains * dof_vel, -lim, lim)
    cmd = torch.zeros(n, 1, nd, device=dev)
    got = glue.actuator_step((actions + default_dof_pos).contiguous(), dof_state, cmd, kp=p_gains, kd=d_gains, delay=0, effort_limit=lim)
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    clipped = float((want.abs() == lim).float().mean())
    assert 0.05 < clipped < 0.95, clipped


# ------------------------------------------------------------------------------------------------------------- facade --
def _a1_env(n, cls):
    from examples.a1_conditional.task_config import A1ActorConfig
    from shifu_amd.configs import BaseEnvConfig
    from shifu_amd.gym.isaac_gym import IsaacGymEnv

    class EnvCfg(BaseEnvConfig):
        num_envs = n

        class debug(BaseEnvConfig.debug):
            headless = True

    np.random.seed(42)                                             # the robot draws its shape frictions at creation
    env = IsaacGymEnv(EnvCfg())
    robot = cls(A1ActorConfig())
    env.create_envs(robot=robot)
    return env, robot


def _robot_classes():
    from examples.a1_conditional.a1_conditional import A1Robot

    class ActuatedA1(A1Robot):
        """A1Robot whose step goes through the robot's actuator instead of the example's torch PD loop."""

        def step(self, actions):
            self.torques = self.apply_actuator_targets(actions + self.default_dof_pos)
            self.post_step()
            self.apply_force_on_base(self.rand_force_buf.view(-1, 3))

    return A1Robot, ActuatedA1


def _state(env):
    return [t.clone() for t in (env.root_state, env.dof_state, env.contact_state, env.body_state)]


def test_facade_pd_actuator_equals_the_examples_step_loop():
    """8 A1 envs on the plane, 20 env steps of `decimation` sub-steps each: apply_actuator_targets (PD, delay 0) leaves the root,
    dof, contact and body tensors the example's A1Robot.step leaves, bit for bit, at every step."""
    _need_gpu()
    from shifu_amd.units import Actuator
    A1Robot, ActuatedA1 = _robot_classes()
    n = 8
    ea, ra = _a1_env(n, A1Robot)
    eb, rb = _a1_env(n, ActuatedA1)
    assert int(ea.decimation) > 1
    rb.set_actuator(Actuator.pd(rb.p_gains, rb.d_gains, effort_limit=rb.torque_limits))
    for env in (ea, eb):
        torch.manual_seed(11)
        env.reset()
    g = torch.Generator(device=ra.device).manual_seed(2)
    for s in range(20):
        actions = 0.5 * (2 * torch.rand(n, 12, device=ra.device, generator=g) - 1)
        ea.step(actions)
        eb.step(actions)
        torch.cuda.synchronize()
        for a, b, name in zip(_state(ea), _state(eb), ("root", "dof", "contact", "body")):
            assert torch.equal(a, b), (name, s)
        assert torch.equal(ra.torques, rb.torques)
    assert torch.isfinite(eb.root_state).all() and torch.isfinite(eb.dof_state).all()
    with pytest.raises(RuntimeError, match="no actuator"):
        ra.apply_actuator_targets(actions)
    ea.destroy(), eb.destroy()


def test_facade_delayed_dc_motor_kernel_equals_the_fallback_and_resets_refill_the_history():
    """The same loop with a delay of two sub-steps and the DC clip: the kernel-backed actuator and the torch fallback leave
    bit-equal tensors at every step.  After reset_idx of half the envs their cmd_hist rows hold the first post-reset target in
    every slot; the other envs' rows are untouched by the reset."""
    _need_gpu()
    from shifu_amd.units import Actuator
    _, ActuatedA1 = _robot_classes()
    n = 8
    envs = [_a1_env(n, ActuatedA1) for _ in range(2)]
    for (env, robot), backend in zip(envs, ("auto", "torch")):
        robot.set_actuator(Actuator.dc_motor(robot.p_gains, robot.d_gains, SAT, VLIM, effort_limit=robot.torque_limits, delay=2, backend=backend))
        torch.manual_seed(11)
        env.reset()
    (ea, ra), (eb, rb) = envs
    assert ra.actuator.uses_kernel(ra.dof_targets) and not rb.actuator.uses_kernel(rb.dof_targets)
    g = torch.Generator(device=ra.device).manual_seed(2)
    ids = torch.tensor([0, 2, 5, 7], device=ra.device)
    rest = torch.tensor([1, 3, 4, 6], device=ra.device)
    for s in range(20):
        actions = 0.5 * (2 * torch.rand(n, 12, device=ra.device, generator=g) - 1)
        if s == 10:
            before = ra.actuator.cmd_hist.clone()
            for env in (ea, eb):
                torch.manual_seed(12)
                env.reset_idx(ids)
            assert torch.equal(ra.actuator.cmd_hist, before) and ra.actuator.pending.tolist() == [1, 0, 1, 0, 0, 1, 0, 1]
            ra.actuator.efforts(actions + ra.default_dof_pos, ea.dof_state)         # one tick outside the env step, on both
            rb.actuator.efforts(actions + rb.default_dof_pos, eb.dof_state)
            first = (actions + ra.default_dof_pos)
            hist = ra.actuator.cmd_hist
            assert torch.equal(hist[ids], first[ids].unsqueeze(1).expand(4, 3, 12)), "every slot holds the first post-reset target"
            assert torch.equal(hist[rest][:, 1:], before[rest][:, :-1]) and torch.equal(hist[rest][:, 0], first[rest]), "the others only shift"
            assert not ra.actuator.any_pending
        ea.step(actions)
        eb.step(actions)
        torch.cuda.synchronize()
        for a, b, name in zip(_state(ea), _state(eb), ("root", "dof", "contact", "body")):
            assert torch.equal(a, b), (name, s)
        assert torch.equal(ra.actuator.cmd_hist, rb.actuator.cmd_hist) and torch.equal(ra.actuator.applied_target, rb.actuator.applied_target)
        assert torch.equal(ra.torques, rb.torques)
    prev = ra.actuator.cmd_hist[:, 0].clone()                     # an env step holds its target for `decimation` sub-steps
    ra.actuator.efforts(prev + 0.1, ea.dof_state)
    assert torch.equal(ra.actuator.applied_target, prev), "a new target is applied two sub-steps late"
    ea.destroy(), eb.destroy()


# ----------------------------------------------------------------------------------------------------------- captured --
def _hip_runtime():
    """The HIP runtime already in the process (torch's)."""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return ctypes.CDLL(line.split()[-1])
    raise RuntimeError("no HIP runtime in the process")


def test_a_captured_call_replays_like_eager_calls_and_is_one_kernel_node():
    """Warm up with one eager call; capture one call and replay it three times; three eager calls from the same starting state
    equal the replays bit for bit, outputs and state.  The graph holds a single node, a kernel."""
    _need_gpu()
    from shifu_amd import glue
    n, nd, L = 65, 12, 4
    net = _net([6, 32, 32, 32, 1], "softsign")
    rng, c, gpu, g, H = _case(n, nd, net, True, L)
    X = R.seeded_call(rng, n, nd)
    target, dof = g(X["target"]), g(np.stack([X["q"], X["qd"]], -1))
    state = lambda: (torch.zeros(n, L, nd, device="cuda:0"), torch.zeros(n, H, nd, device="cuda:0"), torch.zeros(n, H, nd, device="cuda:0"))
    outs = lambda: (torch.zeros(n, nd, device="cuda:0"), torch.zeros(n, nd, device="cuda:0"))

    def call(st, o, reset=None):
        kw = dict(gpu, err_hist=st[1], vel_hist=st[2])
        glue.actuator_step(target, dof, st[0], reset=reset, applied_out=o[0], efforts_out=o[1], **kw)

    ones = torch.ones(n, dtype=torch.uint8, device="cuda:0")
    sa, oa, sb, ob = state(), outs(), state(), outs()
    call(sa, oa, ones)                                              # the warm-up (and resetting) call, on both states
    call(sb, ob, ones)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    start = [t.clone() for t in sa]
    with torch.cuda.graph(graph, stream=side):
        call(sa, oa)
    torch.cuda.current_stream().wait_stream(side)
    hip = _hip_runtime()
    count = ctypes.c_size_t(0)
    raw = ctypes.c_void_p(graph.raw_cuda_graph())
    assert hip.hipGraphGetNodes(raw, None, ctypes.byref(count)) == 0 and count.value == 1, count.value
    node, kind = ctypes.c_void_p(), ctypes.c_int(-1)
    assert hip.hipGraphGetNodes(raw, ctypes.byref(node), ctypes.byref(count)) == 0
    assert hip.hipGraphNodeGetType(node, ctypes.byref(kind)) == 0 and kind.value == 0, "hipGraphNodeTypeKernel"
    graph.instantiate()
    for a, b in zip(sa, start):                                    # capturing ran nothing
        assert torch.equal(a, b)
    for k in range(3):
        graph.replay()
        call(sb, ob)
        torch.cuda.synchronize()
        for a, b in zip(sa + oa, sb + ob):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), k
    assert not torch.equal(sa[1], start[1]), "the replays moved the state on"


# ------------------------------------------------------------------------------------------------- fallback on the GPU --
@pytest.mark.parametrize("kind", ["pd", "dc-motor", "softsign", "tanh", "elu"])
def test_fallback_on_the_gpu_equals_the_kernel(kind):
    """utils.torch_utils.actuator_step on the kernel's own tensors, 20 calls with the state carried on both sides: bit-equal for
    PD and the DC motor.  A network's layers go through a GEMM that sums in its own order, so its efforts are held to the rule of
    the tanh / elu test -- against step64, four times the kernel's measured worst and never above the bound (softsign has no
    library call in it: the bound alone) -- and its states stay bit-equal to the kernel's."""
    _need_gpu()
    from shifu_amd import glue
    from shifu_amd.utils import torch_utils as TU
    n, nd, L = 65, 12, 4
    net = None if kind in ("pd", "dc-motor") else _net([6, 32, 32, 32, 1], kind)
    rng, c, gpu, g, H = _case(n, nd, net, kind != "pd", L)
    z = lambda *s: torch.zeros(*s, device="cuda:0")
    ka = dict(cmd=z(n, L, nd), applied=z(n, nd), out=z(n, nd))
    kb = dict(cmd=z(n, L, nd), applied=z(n, nd), out=z(n, nd))
    hist_b = dict(err_hist=z(n, H, nd), vel_hist=z(n, H, nd)) if net is not None else {}
    s64 = R.new_state(n, nd, L, H, np.float64)
    worst = 0.0
    for k, X, reset in _calls(rng, n, nd):
        dof = g(np.stack([X["q"], X["qd"]], -1))
        r = None if reset is None else g(reset)
        glue.actuator_step(g(X["target"]), dof, ka["cmd"], reset=r, applied_out=ka["applied"], efforts_out=ka["out"], **gpu)
        TU.actuator_step(g(X["target"]), dof, kb["cmd"], reset=r, applied_out=kb["applied"], efforts_out=kb["out"], **dict(gpu, **hist_b))
        torch.cuda.synchronize()
        assert torch.equal(ka["cmd"], kb["cmd"]) and torch.equal(ka["applied"], kb["applied"]), k
        if net is None:
            assert torch.equal(ka["out"].view(torch.int32), kb["out"].view(torch.int32)), k
            continue
        assert torch.equal(gpu["err_hist"], hist_b["err_hist"]) and torch.equal(gpu["vel_hist"], hist_b["vel_hist"]), k
        o64 = R.step64(s64, X["target"], X["q"], X["qd"], **dict(c, reset=reset, net=net))
        taps = list(net["taps"])
        x64 = np.concatenate([net["err_scale"] * s64["err"][:, taps], net["vel_scale"] * s64["vel"][:, taps]], 1).transpose(0, 2, 1).reshape(n * nd, -1)
        b = R.bound(net, x64, c["strength"]).reshape(n, nd)
        tol = b if kind == "softsign" else np.minimum(4.0 * WORST[kind], b)
        d = np.abs(kb["out"].cpu().numpy().astype(np.float64) - o64["efforts"])
        worst = max(worst, float(d.max()))
        assert (d <= tol).all(), (kind, k, float(d.max()), float(tol.min()))
    if net is not None:
        print(f"[actuator gpu] fallback, {kind}: worst |fallback - step64| {worst:.3e} N m")
