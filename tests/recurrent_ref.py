"""Checker for the recurrent policy's sequence entry: the published split-and-pad algorithm (rsl_rl v1.0.2's recurrent
mini-batch), written fresh, float64, CPU.

Each env's T transitions are cut into trajectories after every step whose `dones` flag is set; the trajectories are
padded to a common length and run through torch.nn.LSTM / nn.GRU as one batch; the outputs are un-padded back to (T, N).
A trajectory that starts at t = 0 starts from the carried hidden state of its env; every other trajectory starts right
after a done, where rsl_rl's actor_critic.reset(dones) has zeroed the state: from zero."""
import torch


def split_trajectories(dones):
    """dones (T, N) bool -> list of (env, t0, t1): env's transitions t0 .. t1 - 1 form one trajectory."""
    T, N = dones.shape
    out = []
    for n in range(N):
        t0 = 0
        for t in range(T):
            if bool(dones[t, n]) or t == T - 1:
                out.append((n, t0, t + 1))
                t0 = t + 1
    return out


def run(rnn, obs, dones, hidden):
    """rnn: nn.LSTM / nn.GRU (float64, batch_first=False); obs (T, N, D); dones (T, N); hidden: (h, c) or h, each
    (num_layers, N, H).  Returns the outputs (T, N, H)."""
    T, N, _ = obs.shape
    lstm = isinstance(hidden, (tuple, list))
    hs = tuple(hidden) if lstm else (hidden,)
    trajs = split_trajectories(dones.reshape(T, N) != 0)
    longest = max(t1 - t0 for _, t0, t1 in trajs)
    padded = obs.new_zeros(longest, len(trajs), obs.shape[2])
    init = [h.new_zeros(h.shape[0], len(trajs), h.shape[2]) for h in hs]
    for j, (n, t0, t1) in enumerate(trajs):
        padded[:t1 - t0, j] = obs[t0:t1, n]
        if t0 == 0:
            for dst, src in zip(init, hs):
                dst[:, j] = src[:, n]
    out, _ = rnn(padded, tuple(init) if lstm else init[0])
    # un-pad
    pieces = [[None] * N for _ in range(T)]
    for j, (n, t0, t1) in enumerate(trajs):
        for t in range(t0, t1):
            pieces[t][n] = out[t - t0, j]
    return torch.stack([torch.stack(row) for row in pieces])
