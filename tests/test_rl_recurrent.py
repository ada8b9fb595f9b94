"""Recurrent policies (rl/recurrent.py) on the CPU: the runner accepts ActorCriticRecurrent, rsl_rl's state_dict keys, the
in-sequence reset against the split-and-pad checker (tests/recurrent_ref.py) in float64, reset(dones), hidden-state
carry-over, determinism, and the host-side refusals of the LSTM cell entries."""
import copy
import ctypes

import pytest
import torch

from tests import recurrent_ref
from tests.test_rl import CFG, ReachEnv
from shifu_amd.rl import PPO, ActorCriticRecurrent, Memory, OnPolicyRunner


def _cfg(rnn_type="lstm", layers=1):
    cfg = copy.deepcopy(CFG)
    cfg["runner"]["policy_class_name"] = "ActorCriticRecurrent"
    cfg["policy"].update({"rnn_type": rnn_type, "rnn_hidden_size": 16, "rnn_num_layers": layers})
    return cfg


def test_runner_accepts_the_recurrent_class(tmp_path, capsys):
    torch.manual_seed(0)
    cfg = _cfg()
    cfg["algorithm"]["graph_update"] = True          # not implemented for this class: said once, then updated eagerly
    runner = OnPolicyRunner(ReachEnv(), cfg, log_dir=str(tmp_path), device="cpu")
    ac = runner.alg.actor_critic
    assert isinstance(ac, ActorCriticRecurrent) and ac.is_recurrent
    runner.learn(2)
    assert len(runner.history) == 2
    assert capsys.readouterr().out.count("graph_update is not implemented for recurrent policies") == 1
    assert all(torch.isfinite(torch.tensor([h["value_loss"], h["surrogate_loss"]])).all() for h in runner.history)
    assert runner.get_inference_policy() == ac.act_inference
    with pytest.raises(NotImplementedError):
        bad = _cfg()
        bad["runner"]["policy_class_name"] = "SomethingElse"
        OnPolicyRunner(ReachEnv(), bad, log_dir=None, device="cpu")


@pytest.mark.parametrize("rnn_type,per", [("lstm", 4), ("gru", 3)])
def test_state_dict_has_rsl_rl_names(rnn_type, per):
    D, Dc, A, H, L = 7, 9, 3, 12, 2
    ac = ActorCriticRecurrent(D, Dc, A, actor_hidden_dims=[8], critic_hidden_dims=[8], rnn_type=rnn_type, rnn_hidden_size=H, rnn_num_layers=L)
    sd = ac.state_dict()
    want = {"std": (A,), "actor.0.weight": (8, H), "actor.0.bias": (8,), "actor.2.weight": (A, 8), "actor.2.bias": (A,),
            "critic.0.weight": (8, H), "critic.0.bias": (8,), "critic.2.weight": (1, 8), "critic.2.bias": (1,)}
    for mem, d in (("memory_a", D), ("memory_c", Dc)):
        for l in range(L):
            want[f"{mem}.rnn.weight_ih_l{l}"] = (per * H, d if l == 0 else H)
            want[f"{mem}.rnn.weight_hh_l{l}"] = (per * H, H)
            want[f"{mem}.rnn.bias_ih_l{l}"] = (per * H,)
            want[f"{mem}.rnn.bias_hh_l{l}"] = (per * H,)
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    stock = (torch.nn.LSTM if rnn_type == "lstm" else torch.nn.GRU)(D, H, L)
    ac.memory_a.rnn.load_state_dict(stock.state_dict())
    ac.memory_a.load_state_dict({"rnn." + k: v for k, v in stock.state_dict().items()})
    assert torch.equal(ac.memory_a.rnn.weight_hh_l1, stock.weight_hh_l1)


@pytest.mark.parametrize("layers", [1, 2])
@pytest.mark.parametrize("rnn_type", ["lstm", "gru"])
def test_in_sequence_reset_equals_split_and_pad(rnn_type, layers):
    T, N, D, H = 6, 5, 4, 7
    g = torch.Generator().manual_seed(3)
    mem = Memory(D, type=rnn_type, num_layers=layers, hidden_size=H).double()
    ref = copy.deepcopy(mem.rnn)
    obs = torch.randn(T, N, D, generator=g, dtype=torch.float64)
    dones = torch.rand(T, N, generator=g) < 0.3
    dones[0, 1] = dones[T - 1, 2] = dones[0, 3] = dones[1, 3] = True      # first step, last step, two in a row
    dones[:, 4] = False                                                   # one env whose carried state is used to the end
    k = 2 if rnn_type == "lstm" else 1
    hid = tuple(torch.randn(layers, N, H, generator=g, dtype=torch.float64) for _ in range(k))      # a non-zero carried state
    hidden = hid if rnn_type == "lstm" else hid[0]
    wgt = torch.randn(T * N, H, generator=g, dtype=torch.float64)         # the fixed scalar loss: sum(w * out) + sum(out^2)
    loss_of = lambda o: (wgt * o).sum() + o.square().sum()
    out = mem.forward_sequence(obs, dones, hidden)
    want = recurrent_ref.run(ref, obs, dones, hidden).reshape(T * N, H)
    assert out.shape == want.shape
    err = float((out - want).detach().abs().max())
    print("forward max |diff|", err)
    assert err <= 1e-12
    loss_of(out).backward()
    loss_of(want).backward()
    for (name, p), q in zip(mem.rnn.named_parameters(), ref.parameters()):
        gerr = float((p.grad - q.grad).abs().max())
        print(name, "grad max |diff|", gerr)
        assert gerr <= 1e-12, name
    # uint8 flags as the rollout storage keeps them, and a (T, N, 1) shape, give the same result
    out2 = mem.forward_sequence(obs, dones.to(torch.uint8).unsqueeze(-1), hidden)
    assert torch.equal(out2, out)


@pytest.mark.parametrize("rnn_type", ["lstm", "gru"])
def test_reset_zeroes_exactly_the_finished_rows(rnn_type):
    torch.manual_seed(1)
    N = 6
    ac = ActorCriticRecurrent(3, 3, 2, actor_hidden_dims=[8], critic_hidden_dims=[8], rnn_type=rnn_type, rnn_hidden_size=5, rnn_num_layers=2)
    assert ac.get_hidden_states() == (None, None)
    with torch.no_grad():
        for _ in range(2):
            ac.act(torch.randn(N, 3))
            ac.evaluate(torch.randn(N, 3))
    flat = lambda hs: [t for h in hs for t in (h if isinstance(h, tuple) else (h,))]
    tensors = flat(ac.get_hidden_states())
    assert len(tensors) == (4 if rnn_type == "lstm" else 2) and all(t.shape == (2, N, 5) and t.abs().min() > 0 for t in tensors)
    before = [t.clone() for t in tensors]
    ptrs = [t.data_ptr() for t in tensors]
    dones = torch.tensor([0, 1, 0, 0, 1, 0], dtype=torch.bool)
    ac.reset(dones)
    after = flat(ac.get_hidden_states())
    assert [t.data_ptr() for t in after] == ptrs                         # same buffers: a captured rollout keeps working
    for a, b in zip(after, before):
        assert torch.equal(a[:, ~dones], b[:, ~dones]) and (a[:, dones] == 0).all()
    # advance=False gives the value without stepping the state
    x = torch.randn(N, 3)
    with torch.no_grad():
        v0 = ac.evaluate(x, advance=False)
        assert all(torch.equal(a, b) for a, b in zip(flat(ac.get_hidden_states()), [t.clone() for t in after]))
        v1 = ac.evaluate(x)
    assert torch.equal(v0, v1)
    ac.reset()
    assert all((t == 0).all() for t in flat(ac.get_hidden_states()))


def test_hidden_state_carries_over_and_storage_holds_the_initial_state():
    torch.manual_seed(2)
    N, T = 8, 5
    ac = ActorCriticRecurrent(3, 3, 2, actor_hidden_dims=[8], critic_hidden_dims=[8], rnn_hidden_size=6)
    alg = PPO(ac, num_learning_epochs=1, num_mini_batches=2)
    alg.init_storage(N, T, [3], [None], [2])
    never = torch.zeros(N, dtype=torch.bool)

    def rollout(dones_at_last):
        with torch.no_grad():
            for t in range(T):
                obs = torch.randn(N, 3)
                alg.act(obs, obs)
                alg.process_env_step(torch.randn(N), dones_at_last if t == T - 1 else never, {})
            end = [h.clone() for pair in ac.get_hidden_states() for h in pair]
            alg.compute_returns(torch.randn(N, 3))
            assert all(torch.equal(a, b) for a, b in zip(end, [h for pair in ac.get_hidden_states() for h in pair]))
        return end

    rollout(never)
    st = alg.storage
    assert all((h == 0).all() for h in st.saved_hidden_states_a + st.saved_hidden_states_c)      # the first rollout starts from zero
    alg.update()
    dones = torch.tensor([1, 0, 0, 1, 0, 0, 0, 0], dtype=torch.bool)
    end = rollout(dones)
    assert all((h[:, dones] == 0).all() and h[:, ~dones].abs().min() > 0 for h in end)
    alg.update()
    with torch.no_grad():
        obs = torch.randn(N, 3)
        alg.act(obs, obs)
    saved = list(st.saved_hidden_states_a + st.saved_hidden_states_c)
    assert all(torch.equal(a, b) for a, b in zip(saved, end))              # the state from BEFORE the rollout's first act
    now = [h for pair in ac.get_hidden_states() for h in pair]
    assert not torch.equal(now[0], saved[0])                                 # ... a copy: the live state has moved on


def test_two_recurrent_updates_from_one_seed_are_identical():
    params = []
    for _ in range(2):
        torch.manual_seed(5)
        runner = OnPolicyRunner(ReachEnv(seed=3), _cfg(layers=2), log_dir="", device="cpu")
        runner.log_dir = None
        runner.learn(2)
        params.append([p.detach().clone() for p in runner.alg.actor_critic.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(*params))
    assert all(torch.isfinite(p).all() for p in params[0])
    torch.manual_seed(5)
    fresh = OnPolicyRunner(ReachEnv(seed=3), _cfg(layers=2), log_dir=None, device="cpu").alg.actor_critic
    assert all(not torch.equal(a, b) for a, b in zip(params[0], fresh.parameters()))     # every parameter changed


def test_lstm_entries_refuse_bad_arguments_on_the_host():
    """Overlap, zero sizes and null pointers are refused before any launch: no GPU needed (the pointers are never followed)."""
    from shifu_amd.build import build_native
    build_native()
    from shifu_amd import _lib
    L = _lib.lib()
    err = lambda: L.shf_mlp_last_error().decode()
    M, I, H = 8, 5, 32
    state = 4 * M * H
    x, hp, cp, pack, ho, co, gates = (0x10000000 + 0x100000 * i for i in range(7))
    fwd = lambda x=x, ldx=I, hp=hp, cp=cp, pack=pack, ho=ho, co=co, gates=None, M=M, I=I, H=H: \
        L.shf_lstm_cell_forward(x, ldx, hp, cp, None, pack, None, None, ho, co, gates, M, I, H, None)
    for kw in ({"ho": hp}, {"co": cp}, {"ho": hp + state - 4}, {"co": hp}, {"ho": cp}, {"ho": x}, {"co": ho}, {"gates": ho - 4}):
        assert fwd(**kw) != 0 and "overlap" in err(), kw
    for kw in ({"M": 0}, {"I": 0}, {"H": 0}, {"M": -1}, {"ldx": I - 1}):
        assert fwd(**kw) != 0 and "bad shape" in err(), kw
    for kw in ({"x": None}, {"hp": None}, {"cp": None}, {"pack": None}, {"ho": None}, {"co": None}):
        assert fwd(**kw) != 0 and "null" in err(), kw
    assert fwd(pack=pack + 4) != 0 and "aligned" in err()
    n = ctypes.c_int64()
    assert L.shf_lstm_pack_bytes(0, H, ctypes.byref(n)) != 0 and L.shf_lstm_pack_bytes(I, 0, ctypes.byref(n)) != 0
    assert L.shf_lstm_pack_bytes(I, H, None) != 0 and "shf_lstm_pack_bytes" in err()
    assert L.shf_lstm_pack_bytes(259, 512, ctypes.byref(n)) == 0
    assert n.value == 2 * 16 * 4 * (272 // 16 + 512 // 16) * 64 * 16        # heads + tails, 16 slices x 4 gates, 49 k steps, 1 KB each
    assert L.shf_lstm_pack_weights(None, hp, pack, I, H, None) != 0 and "null" in err()
    assert L.shf_lstm_pack_weights(x, hp, pack, 0, H, None) != 0 and "bad shape" in err()
    bwd = lambda dh=x, g=gates, cp=cp, co=co, dg=pack, dcp=ho, M=M, H=H: L.shf_lstm_cell_backward_pointwise(dh, None, g, cp, None, co, dg, dcp, M, H, None)
    assert bwd(dh=None) != 0 and "null" in err()
    assert bwd(dg=None) != 0 and "null" in err()
    assert bwd(M=0) != 0 and bwd(H=0) != 0 and "bad shape" in err()
