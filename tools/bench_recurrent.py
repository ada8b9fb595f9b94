"""Recurrent-policy benchmark: the fused LSTM cell step (csrc/shf_lstm.hip) against the stock torch.nn.LSTM in the same
process, at the A1 widths (259 -> 512, one layer); --rnn gru: the fused GRU cell step (csrc/shf_gru.hip) against the
stock torch.nn.GRU, same rows.  Times, per call:

    fused_cell / stock_cell      one cell step under no_grad at --rows rows: the kernel with the kept pack / nn.LSTM on a
                                 one-step sequence (no state copy-back in either)
    fused_step / stock_step      Memory.forward: the same plus the copy into the fixed state buffers
    fused_update / stock_update  one PPO update of an ActorCriticRecurrent (MFMA MLPs in both): --minibatches mini-batches of
                                 24 x --mb-envs envs, one epoch, forward + loss + backward + Adam

Each figure is the median over --blocks blocks of --reps calls between device events, the candidates' blocks interleaved,
with the min .. max of the blocks as spread.  One JSON line.

    python tools/bench_recurrent.py [--rnn gru]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def timed(calls, blocks, reps, warmup):
    import torch
    for fn in calls.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(blocks):
        for name, fn in calls.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(reps):
                fn()
            t1.record()
            torch.cuda.synchronize()
            times[name].append(t0.elapsed_time(t1) / reps)
    return {k: dict(ms=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4)) for k, v in times.items()}


def make_update(fused, T, mb, nmb, I, H, dev, rnn="lstm"):
    import torch
    from shifu_amd.rl import PPO, ActorCriticRecurrent
    torch.manual_seed(0)
    ac = ActorCriticRecurrent(I, I, 12, actor_hidden_dims=[512, 256, 128], critic_hidden_dims=[512, 256, 128], rnn_hidden_size=H,
                              mlp_backend="mfma", rnn_fused=fused, rnn_type=rnn)
    alg = PPO(ac, num_learning_epochs=1, num_mini_batches=nmb, device=dev, learning_rate=1e-4, schedule="fixed")
    N = mb * nmb
    alg.init_storage(N, T, [I], [None], [12])
    st = alg.storage
    g = torch.Generator(device=dev).manual_seed(1)
    for t in (st.observations, st.actions, st.rewards, st.values, st.returns, st.advantages, st.mu):
        t.copy_(torch.randn(t.shape, device=dev, generator=g))
    st.sigma.fill_(1.0)
    st.actions_log_prob.copy_(torch.distributions.Normal(st.mu, st.sigma).log_prob(st.actions).sum(-1, keepdim=True))
    st.dones.copy_(torch.rand(T, N, 1, device=dev, generator=g) < 0.02)
    st.save_hidden_states(ac.init_hidden_states(N, dev))
    return alg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--inputs", type=int, default=259)
    ap.add_argument("--hidden", type=int, default=512)
    ap.add_argument("--mb-envs", type=int, default=512)
    ap.add_argument("--minibatches", type=int, default=4)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--blocks", type=int, default=15)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rnn", choices=["lstm", "gru"], default="lstm")
    a = ap.parse_args()
    import torch
    from shifu_amd.rl import Memory
    from shifu_amd.rl.recurrent import gru_cell, lstm_cell
    dev = "cuda:0"
    torch.manual_seed(0)
    M, I, H = a.rows, a.inputs, a.hidden
    fused = Memory(I, type=a.rnn, hidden_size=H, fused=True).to(dev)
    stock = Memory(I, type=a.rnn, hidden_size=H, fused=False).to(dev)
    stock.load_state_dict(fused.state_dict())
    x = torch.randn(M, I, device=dev)
    h0, c0 = torch.randn(1, M, H, device=dev) * 0.5, torch.rand(1, M, H, device=dev) * 2 - 1
    fused.refresh_pack()
    params = fused._layer_params(0)
    if a.rnn == "lstm":
        fused_cell = lambda: lstm_cell(x, h0[0], c0[0], None, *params, fused._pack[0])
        stock_cell = lambda: stock.rnn(x.unsqueeze(0), (h0, c0))
    else:
        fused_cell = lambda: gru_cell(x, h0[0], None, *params, fused._pack[0])
        stock_cell = lambda: stock.rnn(x.unsqueeze(0), h0)
    with torch.no_grad():
        if a.rnn == "lstm":
            hf, cf = fused_cell()
            out, (hs, cs) = stock_cell()
            diff = max(float((hf - hs[0]).abs().max()), float((cf - cs[0]).abs().max()))
        else:
            diff = float((fused_cell() - stock_cell()[1][0]).abs().max())

        def no_grad(fn):
            def run():
                with torch.no_grad():
                    return fn()
            return run
        cell = timed({"fused_cell": no_grad(fused_cell), "stock_cell": no_grad(stock_cell),
                      "fused_step": no_grad(lambda: fused(x)), "stock_step": no_grad(lambda: stock(x))}, a.blocks, a.reps, a.warmup)
    upd = {k: make_update(k == "fused_update", a.steps, a.mb_envs, a.minibatches, I, H, dev, a.rnn) for k in ("fused_update", "stock_update")}
    update = timed({k: alg.update for k, alg in upd.items()}, max(3, a.blocks // 3), 2, 2)
    flop = 2.0 * M * (I + H) * (4 if a.rnn == "lstm" else 3) * H
    print(json.dumps(dict(bench="recurrent", **({} if a.rnn == "lstm" else {"rnn": a.rnn}), rows=M, inputs=I, hidden=H, blocks=a.blocks, reps=a.reps, ms_per_call=cell,
                          speedup_fused_vs_stock_cell=round(cell["stock_cell"]["ms"] / cell["fused_cell"]["ms"], 2),
                          fused_cell_tflops=round(flop / (cell["fused_cell"]["ms"] * 1e-3) / 1e12, 1),
                          fused_vs_stock_max_abs_diff=float(f"{diff:.3g}"),
                          update=dict(steps=a.steps, mb_envs=a.mb_envs, minibatches=a.minibatches, ms_per_update=update,
                                      speedup_fused_vs_stock=round(update["stock_update"]["ms"] / update["fused_update"]["ms"], 2)),
                          device=torch.cuda.get_device_name(0))))


if __name__ == "__main__":
    main()
