"""Recurrent policy: rsl_rl's ActorCriticRecurrent (PPOConfig.policy: rnn_type 'lstm', rnn_hidden_size 512,
rnn_num_layers 1; shifu/configs/policy_config.py:13-16) with static shapes.

rsl_rl v1.0.2 trains its recurrent policy on trajectories cut at `dones`, padded, run through the RNN and un-padded:
data-dependent shapes and a nonzero().  The equivalent form used here runs the RNN over the whole (T, n) block of a
mini-batch from the hidden state the rollout began with, and multiplies h and c of env j by 1 - dones[t - 1, j] before
step t >= 1.  That is exact: rsl_rl zeroes the hidden state of finished envs after every step, so the state a trajectory
starts from is either zero or the carried state at t = 0 (tests/test_rl_recurrent.py against split-and-pad).

`Memory` holds a stock nn.LSTM / nn.GRU named `rnn` (rsl_rl's state_dict keys: memory_a.rnn.weight_ih_l0, ...).  On CUDA
fp32 tensors both can run on a fused cell kernel (`fused=True`) -- csrc/shf_lstm.hip for the LSTM, csrc/shf_gru.hip for
the GRU: one launch per layer and time step, the pointwise update in the GEMM's epilogue, one autograd node per cell
step.  Everything else -- CPU tensors, other dtypes, bias=False -- steps the stock module one time step at a time with
the same reset multiplication: same maths, no native calls."""
import ctypes as C

import torch
import torch.nn as nn

from . import mfma_linear as ml
from .actor_critic import ActorCritic


def _gradient_gemms(x, h_prev, reset, w_ih, w_hh, dgx, dgh, N, need_x, need_h, need_w):
    """What both cells' backward passes do after their pointwise kernel, on the MLP layers' gradient GEMMs and the raw
    weights: from the pre-activation gradients of the x side and of the h side ((M, N) each; the LSTM's are one tensor) to
    (dx, dh_prev, dw_ih, dw_hh, db_ih, db_hh), None where not needed.  db_hh is computed only where dgh is a tensor of its
    own (it equals db_ih otherwise).  `reset`: the cell step's; its rows' h_prev counted as zero, so they take no gradient
    through it.  Called under the tensors' device."""
    L = ml.lib()
    M, I = x.shape
    H = h_prev.shape[1]
    st = ml._stream(x)
    keep = None if reset is None else (1.0 - reset.to(torch.float32)).unsqueeze(1)
    dx = dh_prev = dw_ih = dw_hh = db_ih = db_hh = None
    if need_x:
        dx = torch.empty_like(x)
        ml._check(L.shf_mlp_linear_backward_input(ml._ptr(dgx), None, ml._ptr(w_ih), ml._ptr(dx), M, I, N, st))
    if need_h:
        dh_prev = torch.empty_like(h_prev)
        ml._check(L.shf_mlp_linear_backward_input(ml._ptr(dgh), None, ml._ptr(w_hh), ml._ptr(dh_prev), M, H, N, st))
        if keep is not None:
            dh_prev = dh_prev * keep
    if need_w:
        def workspace(K):
            n = C.c_int64()
            ml._check(L.shf_mlp_backward_weight_workspace(M, K, N, C.byref(n)))
            return torch.empty(n.value, device=x.device, dtype=torch.float32)
        dw_ih, dw_hh = torch.empty_like(w_ih), torch.empty_like(w_hh)
        db_ih = torch.empty(N, device=x.device, dtype=torch.float32)
        db_hh = None if dgh is dgx else torch.empty_like(db_ih)
        ml._check(L.shf_mlp_linear_backward_weight(ml._ptr(dgx), None, ml._ptr(x), ml._ptr(dw_ih), ml._ptr(db_ih), ml._ptr(workspace(I)),
                                                   M, I, N, st))
        h_eff = h_prev if keep is None else h_prev * keep
        ml._check(L.shf_mlp_linear_backward_weight(ml._ptr(dgh), None, ml._ptr(h_eff), ml._ptr(dw_hh), None if db_hh is None else ml._ptr(db_hh),
                                                   ml._ptr(workspace(H)), M, H, N, st))
    return dx, dh_prev, dw_ih, dw_hh, db_ih, db_hh


def _pack_weights(kind, w_ih, w_hh, out):
    """[W_ih | W_hh] in the fragment order of the `kind` ('lstm' / 'gru') cell kernel (shf_<kind>_pack_weights); `out`: a
    kept buffer to refill, or None."""
    L = ml.lib()
    H, I = w_hh.shape[1], w_ih.shape[1]
    with torch.cuda.device(w_ih.device):
        if out is None:
            n = C.c_int64()
            ml._check(getattr(L, f"shf_{kind}_pack_bytes")(I, H, C.byref(n)))
            out = torch.empty(n.value, device=w_ih.device, dtype=torch.uint8)
        ml._check(getattr(L, f"shf_{kind}_pack_weights")(ml._ptr(w_ih), ml._ptr(w_hh), ml._ptr(out), I, H, ml._stream(w_ih)))
    return out


class _LstmCellFn(torch.autograd.Function):
    """One LSTM cell step on shf_lstm_cell_forward; backward = the pointwise kernel + the MLP layers' gradient GEMMs on the
    raw weights.  `reset`: uint8 (M,), nonzero rows take h_prev = c_prev = 0 (or None)."""

    @staticmethod
    def forward(ctx, x, h_prev, c_prev, reset, w_ih, w_hh, b_ih, b_hh, pack):
        L = ml.lib()
        x, h_prev, c_prev = x.contiguous(), h_prev.contiguous(), c_prev.contiguous()
        M, I = x.shape
        H = h_prev.shape[1]
        need = any(ctx.needs_input_grad)
        with torch.cuda.device(x.device):
            if pack is None:
                pack = pack_lstm_weights(w_ih, w_hh)
            h, c = torch.empty_like(h_prev), torch.empty_like(c_prev)
            gates = torch.empty(M, 4 * H, device=x.device, dtype=torch.float32) if need else None
            ml._check(L.shf_lstm_cell_forward(ml._ptr(x), I, ml._ptr(h_prev), ml._ptr(c_prev), None if reset is None else ml._ptr(reset),
                                              ml._ptr(pack), ml._ptr(b_ih), ml._ptr(b_hh), ml._ptr(h), ml._ptr(c),
                                              None if gates is None else ml._ptr(gates), M, I, H, ml._stream(x)))
        if need:
            ctx.save_for_backward(x, h_prev, c_prev, reset, w_ih, w_hh, gates, c)
        return h, c

    @staticmethod
    def backward(ctx, dh, dc):
        L = ml.lib()
        x, h_prev, c_prev, reset, w_ih, w_hh, gates, c = ctx.saved_tensors
        M, I = x.shape
        H = h_prev.shape[1]
        dh, dc = dh.contiguous(), dc.contiguous()
        dgates = torch.empty_like(gates)
        dc_prev = torch.empty_like(c_prev)
        with torch.cuda.device(x.device):
            ml._check(L.shf_lstm_cell_backward_pointwise(ml._ptr(dh), ml._ptr(dc), ml._ptr(gates), ml._ptr(c_prev), None if reset is None else ml._ptr(reset), ml._ptr(c),
                                                         ml._ptr(dgates), ml._ptr(dc_prev), M, H, ml._stream(x)))
            dx, dh_prev, dw_ih, dw_hh, db, _ = _gradient_gemms(x, h_prev, reset, w_ih, w_hh, dgates, dgates, 4 * H, ctx.needs_input_grad[0],
                                                               ctx.needs_input_grad[1], any(ctx.needs_input_grad[4:8]))
        if not ctx.needs_input_grad[2]:
            dc_prev = None
        return dx, dh_prev, dc_prev, None, dw_ih, dw_hh, db, (None if db is None else db.clone()), None


def pack_lstm_weights(w_ih, w_hh, out=None):
    """[W_ih | W_hh] in the cell kernel's fragment order (shf_lstm_pack_weights); `out`: a kept buffer to refill."""
    return _pack_weights("lstm", w_ih, w_hh, out)


def lstm_cell(x, h_prev, c_prev, reset, w_ih, w_hh, b_ih, b_hh, pack=None):
    """(h, c) of one fused LSTM cell step (CUDA fp32; `reset` uint8 (M,) or None; `pack` from pack_lstm_weights or None)."""
    ml._apply_env_precision()
    return _LstmCellFn.apply(x, h_prev, c_prev, reset, w_ih, w_hh, b_ih, b_hh, pack)


class _GruCellFn(torch.autograd.Function):
    """One GRU cell step on shf_gru_cell_forward; backward = the pointwise kernel + the MLP layers' gradient GEMMs on the
    raw weights (N = 3H).  `reset`: uint8 (M,), nonzero rows take h_prev = 0 (or None)."""

    @staticmethod
    def forward(ctx, x, h_prev, reset, w_ih, w_hh, b_ih, b_hh, pack):
        L = ml.lib()
        x, h_prev = x.contiguous(), h_prev.contiguous()
        M, I = x.shape
        H = h_prev.shape[1]
        need = any(ctx.needs_input_grad)
        with torch.cuda.device(x.device):
            if pack is None:
                pack = pack_gru_weights(w_ih, w_hh)
            h = torch.empty_like(h_prev)
            gates = torch.empty(M, 4 * H, device=x.device, dtype=torch.float32) if need else None      # r, z, n, hn
            ml._check(L.shf_gru_cell_forward(ml._ptr(x), I, ml._ptr(h_prev), None if reset is None else ml._ptr(reset), ml._ptr(pack),
                                             ml._ptr(b_ih), ml._ptr(b_hh), ml._ptr(h), None if gates is None else ml._ptr(gates),
                                             M, I, H, ml._stream(x)))
        if need:
            ctx.save_for_backward(x, h_prev, reset, w_ih, w_hh, gates)
        return h

    @staticmethod
    def backward(ctx, dh):
        L = ml.lib()
        x, h_prev, reset, w_ih, w_hh, gates = ctx.saved_tensors
        M, I = x.shape
        H = h_prev.shape[1]
        dh = dh.contiguous()
        dgx = torch.empty(M, 3 * H, device=x.device, dtype=torch.float32)
        dgh = torch.empty_like(dgx)
        dh_direct = torch.empty_like(h_prev)
        with torch.cuda.device(x.device):
            ml._check(L.shf_gru_cell_backward_pointwise(ml._ptr(dh), ml._ptr(gates), ml._ptr(h_prev), None if reset is None else ml._ptr(reset), ml._ptr(dgx), ml._ptr(dgh),
                                                        ml._ptr(dh_direct), M, H, ml._stream(x)))
            dx, dh_prev, dw_ih, dw_hh, db_ih, db_hh = _gradient_gemms(x, h_prev, reset, w_ih, w_hh, dgx, dgh, 3 * H, ctx.needs_input_grad[0],
                                                                      ctx.needs_input_grad[1], any(ctx.needs_input_grad[3:7]))
            if dh_prev is not None:
                dh_prev = dh_prev + dh_direct
        return dx, dh_prev, None, dw_ih, dw_hh, db_ih, db_hh, None


def pack_gru_weights(w_ih, w_hh, out=None):
    """[W_ih | W_hh] in the GRU cell kernel's fragment order (shf_gru_pack_weights); `out`: a kept buffer to refill."""
    return _pack_weights("gru", w_ih, w_hh, out)


def gru_cell(x, h_prev, reset, w_ih, w_hh, b_ih, b_hh, pack=None):
    """h of one fused GRU cell step (CUDA fp32; `reset` uint8 (M,) or None; `pack` from pack_gru_weights or None)."""
    ml._apply_env_precision()
    return _GruCellFn.apply(x, h_prev, reset, w_ih, w_hh, b_ih, b_hh, pack)


class Memory(nn.Module):
    """The RNN in front of an MLP.  Step mode (`forward(x)`, x (N, D)) advances the module's own hidden state, kept in
    fixed buffers (state, next state, copy back) so that addresses are stable under graph capture; sequence mode
    (`forward_sequence`) is the update's entry.

    Kept weight packs follow MfmaLinear's rules: `refresh_pack()` at rollout start, `invalidate_pack()` across the update,
    per call under autograd."""
    _keeps_pack = True        # rl/mfma_linear.py refresh_packs / invalidate_packs / mark_packs_valid

    def __init__(self, input_size, type="lstm", num_layers=1, hidden_size=256, fused=False):
        super().__init__()
        kind = type.lower()
        if kind not in ("lstm", "gru"):
            raise ValueError(f"rnn_type '{type}': 'lstm' or 'gru'")
        self.kind, self.fused = kind, bool(fused)
        self.rnn = (nn.LSTM if kind == "lstm" else nn.GRU)(input_size=input_size, hidden_size=hidden_size, num_layers=num_layers)
        self.hidden_states = None          # tuple of (num_layers, N, H) tensors: (h, c) for LSTM, (h,) for GRU
        self._next = None
        self._pack = None                  # one pack per layer
        self._pack_valid = False

    # ------------------------------------------------------------------ kept packs
    def refresh_pack(self):
        w = self.rnn.weight_ih_l0
        if not (self.fused and w.is_cuda and w.dtype == torch.float32):
            return
        with torch.no_grad():
            if self._pack is None or self._pack[0].device != w.device:
                self._pack = [None] * self.rnn.num_layers
            for l in range(self.rnn.num_layers):
                self._pack[l] = _pack_weights(self.kind, getattr(self.rnn, f"weight_ih_l{l}"), getattr(self.rnn, f"weight_hh_l{l}"), self._pack[l])
        self._pack_valid = True

    def invalidate_pack(self):
        self._pack_valid = False

    def _load_from_state_dict(self, *args, **kwargs):
        self._pack_valid = False
        return super()._load_from_state_dict(*args, **kwargs)

    def _apply(self, fn, *args, **kwargs):
        self._pack_valid = False
        self.hidden_states = self._next = None          # (plain tensors, not buffers: they do not follow; re-made on the next step)
        return super()._apply(fn, *args, **kwargs)

    # ------------------------------------------------------------------ state
    def init_state(self, n, device, dtype):
        hs = self.hidden_states
        if hs is None or hs[0].shape[1] != n or hs[0].device != torch.device(device) or hs[0].dtype != dtype:
            shape = (self.rnn.num_layers, n, self.rnn.hidden_size)
            k = 2 if self.kind == "lstm" else 1
            self.hidden_states = tuple(torch.zeros(shape, device=device, dtype=dtype) for _ in range(k))
            self._next = tuple(torch.zeros(shape, device=device, dtype=dtype) for _ in range(k))
        return self.hidden_states

    def get_hidden_states(self):
        """(h, c) for LSTM, h for GRU (rsl_rl's convention), or None before the first step."""
        if self.hidden_states is None:
            return None
        return self.hidden_states if self.kind == "lstm" else self.hidden_states[0]

    def reset(self, dones=None):
        """Zero the hidden rows of finished envs, by multiplication: no boolean indexing, no host sync, same buffers."""
        if self.hidden_states is None:
            return
        with torch.no_grad():
            for s in self.hidden_states:
                if dones is None:
                    s.zero_()
                else:
                    s.mul_((1 - dones.to(device=s.device, dtype=s.dtype)).view(1, -1, 1))

    def _layer_params(self, l):
        r = self.rnn
        return (getattr(r, f"weight_ih_l{l}"), getattr(r, f"weight_hh_l{l}"), getattr(r, f"bias_ih_l{l}"), getattr(r, f"bias_hh_l{l}"))

    def _use_kernel(self, x):
        return self.fused and x.is_cuda and x.dtype == torch.float32 and self.rnn.bias

    def _cell(self, l, inp, state, reset, pack=None):
        """One fused cell step of layer l from its `state` -- (h, c) for LSTM, (h,) for GRU -- to its new state, same form."""
        if self.kind == "lstm":
            return lstm_cell(inp, state[0], state[1], reset, *self._layer_params(l), pack)
        return (gru_cell(inp, state[0], reset, *self._layer_params(l), pack),)

    # ------------------------------------------------------------------ step mode
    def forward(self, x, masks=None, hidden_states=None, advance=True):
        """x (N, D) -> (N, H), advancing the module's hidden state (advance=False: the output only, state untouched)."""
        if masks is not None or hidden_states is not None:
            raise ValueError("Memory: padded-trajectory batches (masks) are not used by this trainer; the update runs "
                             "forward_sequence(obs (T, n, D), dones (T, n), hidden_states)")
        state = self.init_state(x.shape[0], x.device, x.dtype)
        nxt = self._next
        if self._use_kernel(x):
            inp = x
            packs = self._pack if (self._pack_valid and not torch.is_grad_enabled()) else None
            for l in range(self.rnn.num_layers):
                new = self._cell(l, inp, [s[l] for s in state], None, None if packs is None else packs[l])
                with torch.no_grad():
                    for d, s in zip(nxt, new):
                        d[l].copy_(s)
                inp = new[0]
            out = inp
        else:
            out, new = self.rnn(x.unsqueeze(0), state if self.kind == "lstm" else state[0])
            out = out[0]
            with torch.no_grad():
                for d, s in zip(nxt, new if self.kind == "lstm" else (new,)):
                    d.copy_(s)
        if advance:
            with torch.no_grad():
                for s, d in zip(state, nxt):
                    s.copy_(d)
        return out

    # ------------------------------------------------------------------ sequence mode
    def forward_sequence(self, obs, dones, hidden_states):
        """obs (T, n, D), dones (T, n) (nonzero: the env finished in that step), hidden_states as get_hidden_states()
        returns them ((L, n, H) per tensor) -> (T * n, H), row t * n + j.  The module's own state is not touched."""
        T, n = obs.shape[0], obs.shape[1]
        init = hidden_states if isinstance(hidden_states, (tuple, list)) else (hidden_states,)
        dones = dones.reshape(T, n)
        outs = []
        if self._use_kernel(obs):
            rb = dones.to(torch.uint8)
            state = [[s[l] for s in init] for l in range(self.rnn.num_layers)]
            for t in range(T):
                reset = None if t == 0 else rb[t - 1].contiguous()
                inp = obs[t]
                for l in range(self.rnn.num_layers):
                    state[l] = self._cell(l, inp, state[l], reset)
                    inp = state[l][0]
                outs.append(inp)
            return torch.cat(outs, dim=0)
        state = [s for s in init]
        for t in range(T):
            if t >= 1:
                keep = (1 - dones[t - 1].to(obs.dtype)).view(1, n, 1)
                state = [s * keep for s in state]
            state = [s.contiguous() for s in state]
            out, new = self.rnn(obs[t:t + 1], tuple(state) if self.kind == "lstm" else state[0])
            state = list(new) if self.kind == "lstm" else [new]
            outs.append(out[0])
        return torch.cat(outs, dim=0)


class ActorCriticRecurrent(ActorCritic):
    """memory_a -> actor MLP, memory_c -> critic MLP (rsl_rl's submodule names: memory_a, memory_c, actor, critic, std)."""
    is_recurrent = True

    def __init__(self, num_actor_obs, num_critic_obs, num_actions, actor_hidden_dims=(256, 256, 256),
                 critic_hidden_dims=(256, 256, 256), activation="elu", rnn_type="lstm", rnn_hidden_size=256, rnn_num_layers=1,
                 init_noise_std=1.0, mlp_backend=None, rnn_fused=None, **kwargs):
        if kwargs:
            print("ActorCriticRecurrent: ignoring unknown policy keys " + ", ".join(kwargs))
        super().__init__(rnn_hidden_size, rnn_hidden_size, num_actions, actor_hidden_dims=actor_hidden_dims,
                         critic_hidden_dims=critic_hidden_dims, activation=activation, init_noise_std=init_noise_std,
                         mlp_backend=mlp_backend)
        # the fused LSTM cell goes with the MFMA layers: its step is 3.3 x the stock one's at the A1 widths;
        # rnn_fused=False keeps the stock LSTM next to them (tools/bench_recurrent.py's comparison).  The fused GRU cell
        # (csrc/shf_gru.hip) is chosen with rnn_fused=True only: None keeps the stock nn.GRU
        fused = (self.mlp_backend == "mfma" and rnn_type.lower() == "lstm") if rnn_fused is None else bool(rnn_fused)
        self.memory_a = Memory(num_actor_obs, type=rnn_type, num_layers=rnn_num_layers, hidden_size=rnn_hidden_size, fused=fused)
        self.memory_c = Memory(num_critic_obs, type=rnn_type, num_layers=rnn_num_layers, hidden_size=rnn_hidden_size, fused=fused)

    def reset(self, dones=None):
        self.memory_a.reset(dones)
        self.memory_c.reset(dones)

    def get_hidden_states(self):
        return self.memory_a.get_hidden_states(), self.memory_c.get_hidden_states()

    def init_hidden_states(self, n, device, dtype=torch.float32):
        self.memory_a.init_state(n, device, dtype)
        self.memory_c.init_state(n, device, dtype)
        return self.get_hidden_states()

    def act(self, observations, masks=None, hidden_states=None, **kwargs):
        return super().act(self.memory_a(observations, masks, hidden_states))

    def act_inference(self, observations):
        return self.actor(self.memory_a(observations))

    def evaluate(self, critic_observations, masks=None, hidden_states=None, advance=True, **kwargs):
        """advance=False: the value under the carried state without stepping it (the bootstrap value after a rollout:
        the next rollout's first step sees the same observation again)."""
        return self.critic(self.memory_c(critic_observations, masks, hidden_states, advance=advance))

    def sequence_features(self, obs, critic_obs, dones, hidden_states):
        """The update's entry: obs / critic_obs (T, n, D), dones (T, n), hidden_states = (actor's, critic's) as
        get_hidden_states() gave them before the first step -> the actor MLP's and the critic MLP's inputs, (T * n, H) each."""
        ha, hc = hidden_states
        return self.memory_a.forward_sequence(obs, dones, ha), self.memory_c.forward_sequence(critic_obs, dones, hc)
