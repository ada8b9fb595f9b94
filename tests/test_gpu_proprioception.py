"""The proprioceptive sensors on the GPU (csrc/shf_proprio.hip: shf_proprioception_step) and what stands on them
(glue.proprioception_step, shifu_amd.proprio.Proprioception, FusedA1Env.add_proprioception, units.ProprioceptionSensor).

Kernel against twin.  tests/proprio_ref.py `step32` is the kernel's header in NumPy float32, operation by operation: 20
consecutive reads with the state carried on both sides, two IMUs on different bodies, four feet, per-env delays 0..3 at L = 4,
every noise term on, resets of about 40 % of the envs at reads 5 and 11.  Every output and every state tensor must be bit-equal
at every read.  Against `step64` no number was fixed in advance: WORST below is the largest |kernel - step64| per output class
over every shape and read, measured on an MI355X, and the test asserts four times that.  (The kernel is bit-equal to step32, so
these are float32's distances from float64 on these motions: the accelerometer differences two velocities of a few m/s over
0.02 s, which multiplies their rounding by 50; a quantised position or a switch can land one step away when the value sits on a
rounding boundary, and then the times that follow a switch differ by whole reads.)
"""
import ctypes

import numpy as np
import pytest

from tests import proprio_ref as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

READS = 20
SHAPES = [(1, 12), (63, 5), (64, 12), (65, 5), (257, 12)]     # envs straddle wavefronts; partial last wavefronts; several blocks
NB, L, DT = 6, 4, 0.02
G = (0.0, 0.0, -9.81)
IMUS = [dict(body=0, position=(0.1, -0.05, 0.2), quat=(0.1, 0.2, -0.3, 0.9)), dict(body=4, position=(-0.2, 0.0, 0.05), quat=(0.5, -0.5, 0.5, 0.5))]
FEET = [1, 2, 3, 5]
NOISE = dict(gyro_noise=0.02, accel_noise=0.1, gyro_walk=0.01, accel_walk=0.05, gyro_bias=0.05, accel_bias=0.3, dof_pos_noise=0.005,
             dof_vel_noise=0.1, dof_offset=0.02, resolution=0.001, f_on=6.0, f_off=3.0)
SEED = 0x1234567890ABCDEF
# largest |kernel - step64| per output class, MI355X, all SHAPES x READS (printed by the test; the units are the outputs')
# gyro rad/s; accel m/s^2; dof_pos rad: one encoder step of 0.001 (a single position on a rounding boundary, at 257 x 12; 5.8e-8
# everywhere else); dof_vel rad/s (the differenced velocity; 2.7e-7 measured directly); no switch ever differed; the times s
WORST = {"gyro": 1.440e-6, "accel": 1.398e-5, "dof_pos": 1.000e-3, "dof_vel": 5.169e-6, "contact": 0.0, "first_contact": 0.0,
         "air_time": 4.470e-8, "contact_time": 2.980e-8, "last_air_time": 3.353e-8, "last_contact_time": 3.353e-8}
DEV = "cuda:0"


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible (these tests never fall back to CPU)")


def g(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def delays(gids):
    gids = np.asarray(gids)
    return ((gids[:, None] * np.array([1, 3, 5]) + np.array([0, 1, 2])) % L).astype(np.int32)


def resets_at(k, gids):
    """About 40 % of the envs at reads 5 and 11, a function of the global id."""
    gids = np.asarray(gids)
    if k not in (5, 11):
        return np.zeros(len(gids), np.uint8)
    return ((gids * 7 + k) % 5 < 2).astype(np.uint8)


def _config(nd, velocity="direct", mode="norm", offset=0, **kw):
    from shifu_amd import proprio
    c = proprio.make_config(imus=IMUS, feet=FEET, num_bodies=NB, contact_mode=mode, velocity=velocity, slots=L, gravity=G, dt=DT, seed=SEED,
                            env_id_offset=offset, **kw)
    return c, proprio.make_params(DT, **NOISE)


class Gpu:
    """The kernel's side of a run: state and outputs on the device."""

    def __init__(self, n, nd, c, params):
        from shifu_amd import proprio
        self.n, self.nd, self.c, self.params = n, nd, c, params.to(DEV)
        self.state = proprio.make_state(n, c.num_imus, nd, c.num_feet, c.slots, DEV)
        self.out = torch.zeros(n, proprio.out_width(c.num_imus, nd, c.num_feet), device=DEV)
        self.sw = torch.zeros(n, 2 * c.num_feet, dtype=torch.uint8, device=DEV)

    def read(self, body, dof, con, delay, reset, gids=None):
        from shifu_amd import glue
        as_t = lambda a: a if torch.is_tensor(a) else g(a)
        glue.proprioception_step(as_t(body), as_t(dof), as_t(con), self.c, self.params, as_t(delay), self.state, self.out, self.sw,
                                 None if reset is None else as_t(reset), None if gids is None else as_t(np.asarray(gids, np.int64)))
        torch.cuda.synchronize()
        return self.out.cpu().numpy(), self.sw.cpu().numpy()


def _run_gpu(gids, nd, c, params, explicit_ids=False, reads=READS):
    """READS reads of the envs `gids` (their motions, delays and resets are functions of the global id): the outputs per read."""
    gpu = Gpu(len(gids), nd, c, params)
    outs = []
    for k in range(reads):
        body, dof, con = R.synthetic(gids, NB, nd, k, DT)
        outs.append(gpu.read(body, dof, con, delays(gids), resets_at(k, gids), gids if explicit_ids else None))
    return outs, gpu


# ------------------------------------------------------------------------------------------------- kernel against twin --
@pytest.mark.parametrize("n,nd,velocity,mode", [(n, nd, "direct", "norm") for n, nd in SHAPES] + [(65, 5, "difference", "z")])
def test_kernel_equals_the_twin_bit_for_bit_and_stands_this_far_from_float64(n, nd, velocity, mode):
    _need_gpu()
    offset = (1 << 32) - 11                                        # global ids on both sides of 2^32: the counter's fourth word
    c, params = _config(nd, velocity, mode, offset)
    cfg = R.config_of(c)
    gids = offset + np.arange(n)
    gpu = Gpu(n, nd, c, params)
    s32 = R.make_state(n, 2, nd, 4, L)
    s64 = R.make_state(n, 2, nd, 4, L, np.float64)
    worst = {k: 0.0 for k in WORST}
    seen = np.zeros((2, 8), bool)
    for k in range(READS):
        body, dof, con = R.synthetic(gids, NB, nd, k, DT)
        rs, dl = resets_at(k, gids), delays(gids)
        out, sw = gpu.read(body, dof, con, dl, rs)
        want, want_sw = R.step32(cfg, params.numpy(), s32, body, dof, con, dl, rs)
        assert np.array_equal(_bits(out), _bits(want)), (k, np.argwhere(_bits(out) != _bits(want))[:5])
        assert np.array_equal(sw, want_sw), k
        for name in ("counter", "imu", "enc", "foot"):
            assert np.array_equal(_bits(gpu.state[name]), _bits(s32[name])), (k, name)
        seen[0] |= (sw == 0).any(0)
        seen[1] |= (sw == 1).any(0)
        ref, _ = R.step64(cfg, params.numpy(), s64, body, dof, con, dl, rs)
        a, b = R.split(out.astype(np.float64), 2, nd, 4), R.split(ref, 2, nd, 4)
        for name in worst:
            worst[name] = max(worst[name], float(np.abs(a[name] - b[name]).max()))
    if n >= 63:
        assert seen.all(), "every switch and every touch-down flag was both 0 and 1"
    print(f"[proprio gpu] {n} x {nd} {velocity} {mode}: worst |kernel - step64| " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    for name, v in worst.items():
        assert WORST[name] is not None, f"no measured figure for {name} yet (this run: {v:.3e})"
        assert v <= 4.0 * WORST[name], (name, v, WORST[name])


# ------------------------------------------------------------------------------------- rows depend on the global id alone --
def test_an_env_alone_among_19_and_permuted_gives_bit_equal_rows():
    """The same global ids as a batch of 19 from env_id_offset, one env at a time, and in permuted order (the ids named by the
    global_ids tensor): every read's rows are bit-equal."""
    _need_gpu()
    nd, base = 12, 1000
    gids = base + np.arange(19)
    c, params = _config(nd, offset=base)
    full, _ = _run_gpu(gids, nd, c, params)
    for e in (0, 7, 18):
        c1, _ = _config(nd, offset=base + e)
        alone, _ = _run_gpu(gids[e:e + 1], nd, c1, params)
        for k in range(READS):
            assert np.array_equal(_bits(alone[k][0][0]), _bits(full[k][0][e])) and np.array_equal(alone[k][1][0], full[k][1][e]), (e, k)
    perm = np.random.default_rng(0).permutation(19)
    c2, _ = _config(nd, offset=0)
    mixed, _ = _run_gpu(gids[perm], nd, c2, params, explicit_ids=True)
    for k in range(READS):
        assert np.array_equal(_bits(mixed[k][0]), _bits(full[k][0][perm])) and np.array_equal(mixed[k][1], full[k][1][perm]), k


def test_two_shards_equal_the_unsharded_run():
    _need_gpu()
    n, nd = 65, 5
    gids = np.arange(n)
    c, params = _config(nd)
    full, gf = _run_gpu(gids, nd, c, params)
    cut = 31
    parts = []
    for lo, hi in ((0, cut), (cut, n)):
        cs, _ = _config(nd, offset=lo)
        parts.append(_run_gpu(gids[lo:hi], nd, cs, params))
    for k in range(READS):
        out = np.concatenate([parts[0][0][k][0], parts[1][0][k][0]])
        sw = np.concatenate([parts[0][0][k][1], parts[1][0][k][1]])
        assert np.array_equal(_bits(out), _bits(full[k][0])) and np.array_equal(sw, full[k][1]), k
    for name in ("counter", "imu", "enc", "foot"):
        both = torch.cat([parts[0][1].state[name], parts[1][1].state[name]])
        assert np.array_equal(_bits(both), _bits(gf.state[name])), name


def test_strided_views_equal_contiguous_copies():
    """The inputs as views into wider tensors (more bodies and dofs per env than the sensor reads, a longer row): as the fused
    envs' and the facade's state tensors are."""
    _need_gpu()
    n, nd = 65, 5
    gids = np.arange(n)
    c, params = _config(nd)
    a, b = Gpu(n, nd, c, params), Gpu(n, nd, c, params)
    for k in range(8):
        body, dof, con = R.synthetic(gids, NB, nd, k, DT)
        wide_body = torch.full((n, NB + 3, 16), 7.0, device=DEV)
        wide_dof = torch.full((n, nd + 2, 3), 7.0, device=DEV)
        wide_con = torch.full((n, NB + 3, 4), 7.0, device=DEV)
        wide_body[:, :NB, :13], wide_dof[:, :nd, :2], wide_con[:, :NB, :3] = g(body), g(dof), g(con)
        vb, vd, vc = wide_body[:, :NB, :13], wide_dof[:, :nd, :2], wide_con[:, :NB, :3]
        assert not vb.is_contiguous() and not vd.is_contiguous() and not vc.is_contiguous()
        rs, dl = resets_at(k + 3, gids), delays(gids)
        oa = a.read(vb, vd, vc, dl, rs)
        ob = b.read(body, dof, con, dl, rs)
        assert np.array_equal(_bits(oa[0]), _bits(ob[0])) and np.array_equal(oa[1], ob[1]), k
    for name in ("counter", "imu", "enc", "foot"):
        assert torch.equal(a.state[name], b.state[name]), name


# ----------------------------------------------------------------------------------------------------------- captured --
def _hip_runtime():
    """The HIP runtime already in the process (torch's)."""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return ctypes.CDLL(line.split()[-1])
    raise RuntimeError("no HIP runtime in the process")


def test_a_captured_read_is_one_kernel_node_and_replays_like_eager_reads():
    """Warm up with one eager read; capture one read and replay it three times; three eager reads from the same starting state
    equal the replays bit for bit, outputs and state: the read counter lives on the device, so every replay draws new noise."""
    _need_gpu()
    from shifu_amd import glue
    n, nd = 65, 12
    gids = np.arange(n)
    c, params = _config(nd)
    a, b = Gpu(n, nd, c, params), Gpu(n, nd, c, params)
    body, dof, con = (g(x) for x in R.synthetic(gids, NB, nd, 3, DT))
    dl = g(delays(gids))

    def call(s):
        glue.proprioception_step(body, dof, con, c, s.params, dl, s.state, s.out, s.sw, None)

    call(a)
    call(b)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    start = {k: v.clone() for k, v in a.state.items()}
    with torch.cuda.graph(graph, stream=side):
        call(a)
    torch.cuda.current_stream().wait_stream(side)
    hip = _hip_runtime()
    count = ctypes.c_size_t(0)
    raw = ctypes.c_void_p(graph.raw_cuda_graph())
    assert hip.hipGraphGetNodes(raw, None, ctypes.byref(count)) == 0 and count.value == 1, count.value
    node, kind = ctypes.c_void_p(), ctypes.c_int(-1)
    assert hip.hipGraphGetNodes(raw, ctypes.byref(node), ctypes.byref(count)) == 0
    assert hip.hipGraphNodeGetType(node, ctypes.byref(kind)) == 0 and kind.value == 0, "hipGraphNodeTypeKernel"
    graph.instantiate()
    for k, v in a.state.items():                                   # capturing ran nothing
        assert torch.equal(v, start[k])
    last = None
    for k in range(3):
        graph.replay()
        call(b)
        torch.cuda.synchronize()
        for name in a.state:
            assert torch.equal(a.state[name], b.state[name]), (k, name)
        assert torch.equal(a.out.view(torch.int32), b.out.view(torch.int32)) and torch.equal(a.sw, b.sw), k
        assert last is None or not torch.equal(a.out[:, :6], last), "a replay draws new noise"
        last = a.out[:, :6].clone()
    assert (a.state["counter"][:, :, 0] == 4).all()


# ------------------------------------------------------------------------------------------------------- the fused env --
def _rotate_inverse64(q, v):
    x, y, z, w = (q[:, k].astype(np.float64) for k in range(4))
    u = np.stack([-x, -y, -z], -1)
    return v + 2.0 * np.cross(u, np.cross(u, v) + w[:, None] * v)


def test_fused_a1_env_reads_what_the_twin_reads_on_the_env_s_own_tensors():
    """FusedA1Env(64 envs, 0.3 s episodes) so that resets happen inside the fused step; 30 step_random() calls, a read of two
    sensors after each.  The noisy one (latency, every noise term) is bit-equal to step32 fed with the env's tensors and the
    reset flags the env's reset counter implies.  The quiet one (no noise, offset, resolution or delay; f_on = f_off = 1 on
    f_z): dof_pos is the dof tensor, the switch is `contact z > 1`, and on the read after a reset the accelerometer reads
    R^T (-g) -- to 1e-5 m/s^2 of a float64 rotation by the float32 quaternion: one rotation-matrix entry is 2 (ab +- cd) with
    |error| <= 3 x 2^-24, times 9.81, plus the quaternion's own distance from unit length (2^-23) times 9.81."""
    _need_gpu()
    from shifu_amd import _abi
    from shifu_amd.gym.a1_fused import FusedA1Env
    n = 64
    env = FusedA1Env(num_envs=n, episode_length_s=0.3)
    nd, B = int(env.cm.blob.nd), env.cam_seg.shape[1]
    dl = torch.from_numpy(delays(np.arange(n))).to(DEV)
    noisy = env.add_proprioception(imu=[dict(body=0, position=(0.1, -0.05, 0.02), quat=(0.1, 0.2, -0.3, 0.9))], feet="auto", max_delay=L - 1,
                                   delay=dl, seed=SEED, **NOISE)
    quiet = env.add_proprioception(imu=[dict(body=0)], feet="auto", contact_mode="z", f_on=1.0, f_off=1.0)
    feet = [b for b, name in enumerate(env.cm.body_names) if name.endswith("_foot")]
    assert len(feet) == 4 and noisy.core.config.num_feet == 4 and abs(noisy.core.dt - env.dt) < 1e-12
    cfg = R.config_of(noisy.core.config)
    assert cfg["feet"] == feet and cfg["gravity"] == tuple(float(v) for v in env.sim_params.gravity)
    s32 = R.make_state(n, 1, nd, 4, L)
    count = env.task.tensors[_abi.A1_RESET_COUNT]
    seen = count.clone()
    grav = np.array([np.float32(v) for v in env.sim_params.gravity], np.float64)
    resets = switched = 0
    for k in range(30):
        env.step_random()
        moved = (count != seen).cpu().numpy()
        seen.copy_(count)
        flags = moved | (k == 0)
        resets += int(moved.sum())
        body = env.body_state.view(n, B, 13).cpu().numpy()
        dof = env.dof_state.view(n, nd, 2).cpu().numpy()
        con = env.contact_state.view(n, B, 3).cpu().numpy()
        o = noisy.read()
        q = quiet.read()
        torch.cuda.synchronize()
        assert np.array_equal(noisy.last_reset.cpu().numpy() != 0, flags), k
        want, want_sw = R.step32(cfg, noisy.core.params.cpu().numpy(), s32, body, dof, con, dl.cpu().numpy(), flags.astype(np.uint8))
        assert np.array_equal(_bits(noisy.flat), _bits(want)), k
        assert np.array_equal(o["contact"].cpu().numpy(), want_sw[:, :4]) and np.array_equal(o["first_contact"].cpu().numpy(), want_sw[:, 4:]), k
        assert o["gyro"].shape == (n, 1, 3) and o["dof_pos"].shape == (n, nd) and o["air_time"].shape == (n, 4)
        assert o["gyro"].data_ptr() == noisy.flat.data_ptr(), "the dict entries are views of the packed tensor"
        # the quiet sensor
        assert torch.equal(q["dof_pos"], env.dof_state.view(n, nd, 2)[:, :, 0]), k
        assert torch.equal(q["dof_vel"], env.dof_state.view(n, nd, 2)[:, :, 1]), k
        assert np.array_equal(q["contact"].cpu().numpy() != 0, con[:, feet, 2] > 1.0), k
        switched += int(q["first_contact"].sum())
        if flags.any():
            rest = _rotate_inverse64(body[flags, 0, 3:7], np.broadcast_to(-grav, (int(flags.sum()), 3)))
            err = np.abs(q["accel"].cpu().numpy()[flags, 0].astype(np.float64) - rest).max()
            assert err <= 1e-5, (k, err)
    assert resets >= n, f"only {resets} resets inside the fused step"
    assert switched > 0, "no foot touched down"
    env.destroy()


# ---------------------------------------------------------------------------------------------------------- the facade --
def _a1_env(n, sensor):
    from examples.a1_conditional.a1_conditional import A1Robot
    from examples.a1_conditional.task_config import A1ActorConfig
    from shifu_amd.configs import BaseEnvConfig
    from shifu_amd.gym.isaac_gym import IsaacGymEnv

    class EnvCfg(BaseEnvConfig):
        num_envs = n

        class debug(BaseEnvConfig.debug):
            headless = True

    np.random.seed(42)                                             # the robot draws its shape frictions at creation
    env = IsaacGymEnv(EnvCfg())
    robot = A1Robot(A1ActorConfig())
    env.create_envs(robot=robot, sensors=[sensor])
    return env, robot


def test_facade_sensor_kernel_equals_the_torch_fallback_also_after_reset_idx():
    """8 A1 envs through the facade, 16 env steps with a read after each and reset_idx of half the envs before step 8: the
    kernel-backed units.ProprioceptionSensor and the one with backend = "torch" leave bit-equal outputs and states."""
    _need_gpu()
    from shifu_amd.configs import ProprioceptionSensorConfig
    from shifu_amd.units import ProprioceptionSensor

    def make(which):
        class Cfg(ProprioceptionSensorConfig):
            name = "proprio"
            imu = [dict(body="base", position=(0.1, -0.05, 0.02), quat=(0.1, 0.2, -0.3, 0.9))]
            feet = "auto"
            max_delay = 2
            delay = (2, 1, 0)
            seed = 5
            backend = which
        for k, v in NOISE.items():
            setattr(Cfg, k, v)
        return _a1_env(8, ProprioceptionSensor(Cfg()))

    (ea, ra), (eb, rb) = make("auto"), make("torch")
    sa, sb = ea.sensors[0], eb.sensors[0]
    assert sa.core.uses_kernel(ea.dof_state) and not sb.core.uses_kernel(eb.dof_state)
    assert sa.core.config.num_feet == 4 and ra.proprioception_sensors == [sa]
    for env in (ea, eb):
        torch.manual_seed(11)
        env.reset()
    ids = torch.tensor([0, 2, 5, 7], device=ea.device)
    gen = torch.Generator().manual_seed(3)
    moved = False
    for k in range(16):
        actions = 0.3 * (torch.rand(8, 12, generator=gen) - 0.5).to(ea.device)
        if k == 8:
            for env in (ea, eb):
                torch.manual_seed(12)
                env.reset_idx(ids)
            assert sa.core.pending.tolist() == [1, 0, 1, 0, 0, 1, 0, 1] and sb.core.pending.tolist() == sa.core.pending.tolist()
        ea.step(actions)
        eb.step(actions)
        oa, ob = sa.read(), sb.read()
        torch.cuda.synchronize()
        assert torch.equal(ea.body_state, eb.body_state) and torch.equal(ea.contact_state, eb.contact_state), k
        assert torch.equal(sa.flat.view(torch.int32), sb.flat.view(torch.int32)), k
        for name in oa:
            assert torch.equal(oa[name], ob[name]), (k, name)
        for name in sa.core.state:
            assert torch.equal(sa.core.state[name], sb.core.state[name]), (k, name)
        assert not sa.core.pending.any()
        if k == 8:
            assert sa.core.last_reset.tolist() == [1, 0, 1, 0, 0, 1, 0, 1]
        moved = moved or bool(oa["contact"].any())
    assert moved and float(oa["accel"].abs().max()) > 1.0
