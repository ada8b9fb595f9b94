"""The GRU path of the recurrent policy (rl/recurrent.py, csrc/shf_gru.hip) without a GPU: `fused=True` is kept for a GRU
Memory and falls back to the stock module on CPU tensors bit for bit, the C ABI declares and binds the four shf_gru_*
entries at version 22, ActorCriticRecurrent's defaults and state_dict names, the host-side refusals of the entries, and
the backward formulas the pointwise kernel implements, transcribed in float64 torch and checked against autograd."""
import ctypes
import os
import re

import pytest
import torch

from shifu_amd.rl import ActorCriticRecurrent, Memory

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["shf_gru_pack_bytes", "shf_gru_pack_weights", "shf_gru_cell_forward", "shf_gru_cell_backward_pointwise"]


def test_fused_gru_memory_on_cpu_tensors_takes_the_stock_branch():
    torch.manual_seed(0)
    D, H, N, T = 8, 16, 5, 4
    mem = Memory(D, type="gru", hidden_size=H, fused=True)
    assert mem.fused is True and mem.kind == "gru"
    stock = torch.nn.GRU(D, H)
    stock.load_state_dict(mem.rnn.state_dict())
    h = torch.zeros(1, N, H)
    with torch.no_grad():
        for _ in range(3):                                  # step mode: the carried state advances
            x = torch.randn(N, D)
            out = mem(x)
            want, h = stock(x.unsqueeze(0), h)
            assert torch.equal(out, want[0]) and torch.equal(mem.get_hidden_states(), h)
        obs, dones = torch.randn(T, N, D), torch.rand(T, N) < 0.4
        hid = torch.randn(1, N, H)
        got = mem.forward_sequence(obs, dones, hid)
        hh, outs = hid, []
        for t in range(T):
            if t >= 1:
                hh = hh * (1 - dones[t - 1].float()).view(1, N, 1)
            o, hh = stock(obs[t:t + 1], hh.contiguous())
            outs.append(o[0])
        assert torch.equal(got, torch.cat(outs, dim=0))
    assert mem._pack is None                                # no native call was made
    mem.refresh_pack()                                      # (a CPU module keeps no pack)
    assert mem._pack is None and not mem._pack_valid


def test_header_and_bindings_declare_the_gru_entries_at_abi_22():
    from shifu_amd import _abi, _lib
    hdr = open(os.path.join(ROOT, "include", "shifu_amd.h")).read()
    for name in ENTRIES:
        assert re.search(r"^int " + name + r"\(", hdr, re.M), name + " is not declared in include/shifu_amd.h"
        assert name in _lib._SIGS and name in _lib.EXPORTS, name
    assert len(_lib._SIGS["shf_gru_cell_forward"][0]) == 13 and len(_lib._SIGS["shf_gru_cell_backward_pointwise"][0]) == 10
    version = int(re.search(r"#define SHF_ABI_VERSION (\d+)", hdr).group(1))
    assert version == 22 and _abi.SHF_ABI_VERSION == 22


def test_policy_defaults_and_state_dict_names():
    D, Dc, A, H, L = 7, 9, 3, 12, 2
    kw = dict(actor_hidden_dims=[8], critic_hidden_dims=[8], rnn_type="gru", rnn_hidden_size=H, rnn_num_layers=L)
    ac = ActorCriticRecurrent(D, Dc, A, mlp_backend=None, **kw)
    assert ac.memory_a.fused is False and ac.memory_c.fused is False
    assert ActorCriticRecurrent(D, Dc, A, mlp_backend=None, rnn_fused=False, **kw).memory_a.fused is False
    on = ActorCriticRecurrent(D, Dc, A, mlp_backend=None, rnn_fused=True, **kw)
    assert on.memory_a.fused is True and on.memory_c.fused is True
    want = {"std", "actor.0.weight", "actor.0.bias", "actor.2.weight", "actor.2.bias",
            "critic.0.weight", "critic.0.bias", "critic.2.weight", "critic.2.bias"}
    for mem in ("memory_a", "memory_c"):
        for l in range(L):
            want |= {f"{mem}.rnn.{p}_l{l}" for p in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")}
    assert set(ac.state_dict()) == want and set(on.state_dict()) == want
    on.load_state_dict(ac.state_dict())
    assert on.memory_a.rnn.weight_ih_l0.shape == (3 * H, D)
    # the LSTM's default is untouched: None follows the MLP backend
    assert ActorCriticRecurrent(D, Dc, A, mlp_backend=None, **dict(kw, rnn_type="lstm")).memory_a.fused is False


def _forward64(x, h, reset, w_ih, w_hh, b_ih, b_hh):
    """The cell's forward equations in float64 (csrc/shf_gru.hip's header): h', and (r, z, n, hn, he)."""
    H = h.shape[1]
    rho = torch.ones(h.shape[0], 1, dtype=h.dtype) if reset is None else (1.0 - reset.to(h.dtype)).unsqueeze(1)
    he = h * rho
    gx, gh = x @ w_ih.t() + b_ih, he @ w_hh.t() + b_hh
    r = torch.sigmoid(gx[:, :H] + gh[:, :H])
    z = torch.sigmoid(gx[:, H:2 * H] + gh[:, H:2 * H])
    hn = gh[:, 2 * H:]
    n = torch.tanh(gx[:, 2 * H:] + r * hn)
    return (1 - z) * n + z * he, (r, z, n, hn, he, rho)


@pytest.mark.parametrize("with_reset", [False, True])
def test_backward_formulas_match_float64_autograd(with_reset):
    """shf_gru_cell_backward_pointwise's formulas and the gradient GEMMs behind it, written out in float64."""
    M, I, H = 3, 4, 5
    g = torch.Generator().manual_seed(11)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    x, h = rnd(M, I), rnd(M, H)
    w_ih, w_hh, b_ih, b_hh = rnd(3 * H, I) * 0.5, rnd(3 * H, H) * 0.5, rnd(3 * H) * 0.5, rnd(3 * H) * 0.5
    reset = torch.tensor([1, 0, 1], dtype=torch.uint8) if with_reset else None
    dh = rnd(M, H)
    leaves = [t.requires_grad_(True) for t in (x, h, w_ih, w_hh, b_ih, b_hh)]
    out, _ = _forward64(x, h, reset, w_ih, w_hh, b_ih, b_hh)
    # the forward equations are torch.nn.GRU's
    stock = torch.nn.GRU(I, H).double()
    with torch.no_grad():
        for p, v in zip(stock.parameters(), (w_ih, w_hh, b_ih, b_hh)):
            p.copy_(v)
        he0 = h if reset is None else h * (1.0 - reset.double()).unsqueeze(1)
        assert float((stock(x.unsqueeze(0), he0.unsqueeze(0))[0][0] - out).abs().max()) <= 1e-12
    (dh * out).sum().backward()
    with torch.no_grad():
        _, (r, z, n, hn, he, rho) = _forward64(x, h, reset, w_ih, w_hh, b_ih, b_hh)
        dn_pre = dh * (1 - z) * (1 - n * n)
        dz_pre = dh * (he - n) * z * (1 - z)
        dr_pre = dn_pre * hn * r * (1 - r)
        dgx = torch.cat([dr_pre, dz_pre, dn_pre], dim=1)
        dgh = torch.cat([dr_pre, dz_pre, dn_pre * r], dim=1)
        dh_direct = dh * z * rho
        got = [dgx @ w_ih, (dgh @ w_hh) * rho + dh_direct, dgx.t() @ x, dgh.t() @ he, dgx.sum(0), dgh.sum(0)]
    for name, a, leaf in zip(["dx", "dh_prev", "dW_ih", "dW_hh", "db_ih", "db_hh"], got, leaves):
        err = float((a - leaf.grad).abs().max())
        print(name, "max |diff|", err)
        assert err <= 1e-12, name
    if with_reset:
        assert (got[1][reset.bool()] == 0).all()


def test_gru_entries_refuse_bad_arguments_on_the_host():
    """Overlap, zero sizes, null pointers and a misaligned pack are refused before any launch: no GPU needed (the pointers
    are never followed)."""
    from shifu_amd.build import build_native
    build_native()
    from shifu_amd import _lib
    L = _lib.lib()
    err = lambda: L.shf_mlp_last_error().decode()
    M, I, H = 8, 5, 32
    state = 4 * M * H
    x, hp, pack, ho, gates, a, b = (0x10000000 + 0x100000 * i for i in range(7))
    fwd = lambda x=x, ldx=I, hp=hp, pack=pack, ho=ho, gates=None, M=M, I=I, H=H: \
        L.shf_gru_cell_forward(x, ldx, hp, None, pack, None, None, ho, gates, M, I, H, None)
    for kw in ({"ho": hp}, {"ho": hp + state - 4}, {"ho": hp - state + 4}, {"ho": x}, {"gates": ho - 4}, {"gates": hp}, {"gates": x}):
        assert fwd(**kw) != 0 and "overlap" in err(), kw
    for kw in ({"M": 0}, {"I": 0}, {"H": 0}, {"M": -1}, {"ldx": I - 1}):
        assert fwd(**kw) != 0 and "bad shape" in err(), kw
    for kw in ({"x": None}, {"hp": None}, {"pack": None}, {"ho": None}):
        assert fwd(**kw) != 0 and "null" in err(), kw
    assert fwd(pack=pack + 4) != 0 and "aligned" in err()
    n = ctypes.c_int64()
    assert L.shf_gru_pack_bytes(0, H, ctypes.byref(n)) != 0 and L.shf_gru_pack_bytes(I, 0, ctypes.byref(n)) != 0
    assert L.shf_gru_pack_bytes(I, H, None) != 0 and "shf_gru_pack_bytes" in err()
    assert L.shf_gru_pack_bytes(259, 512, ctypes.byref(n)) == 0
    assert n.value == 2 * 16 * 3 * (272 // 16 + 512 // 16) * 64 * 16        # heads + tails, 16 slices x 3 gates, 49 k steps, 1 KB each
    assert L.shf_gru_pack_weights(None, hp, pack, I, H, None) != 0 and "null" in err()
    assert L.shf_gru_pack_weights(x, hp, pack, 0, H, None) != 0 and "bad shape" in err()
    assert L.shf_gru_pack_weights(x, hp, pack + 8, I, H, None) != 0 and "aligned" in err()
    bwd = lambda dh=x, g=gates, hp=hp, dgx=a, dgh=b, dd=ho, M=M, H=H: L.shf_gru_cell_backward_pointwise(dh, g, hp, None, dgx, dgh, dd, M, H, None)
    for kw in ({"dh": None}, {"g": None}, {"hp": None}, {"dgx": None}, {"dgh": None}, {"dd": None}):
        assert bwd(**kw) != 0 and "null" in err(), kw
    assert bwd(M=0) != 0 and bwd(H=0) != 0 and "bad shape" in err()
