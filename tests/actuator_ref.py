"""The twin of csrc/shf_actuator.hip (shf_actuator_step): the algorithm of that file's header in NumPy, operation by operation,
every array operation below standing for the same operation on each (env, dof) pair.

    step32   float32: what the kernel computes, bit for bit (softsign and relu; tanh and elu go through the maths library)
    step64   the same text in float64
    bound    the worst-case forward error of the float32 network against step64, from the actual weights

A state is a dict: cmd (n, L, nd), and for a network err and vel (n, H, nd).  A net is a dict: layers [(W (out, in), b (out)),
...], activation, taps, err_scale, vel_scale, out_scale."""
import numpy as np

U = 2.0 ** -24                     # float32 unit roundoff
ACTIVATIONS = ("softsign", "relu", "tanh", "elu")


def new_state(n, nd, L, H=None, dtype=np.float32):
    st = {"cmd": np.zeros((n, L, nd), dtype)}
    if H is not None:
        st["err"], st["vel"] = np.zeros((n, H, nd), dtype), np.zeros((n, H, nd), dtype)
    return st


def make_net(widths, activation="softsign", taps=(0, 1, 2), err_scale=1.0, vel_scale=1.0, out_scale=1.0, seed=0, gain=1.0):
    """A seeded net of the given widths (inputs .. 1): weights uniform in +-gain / sqrt(fan-in), float32."""
    rng = np.random.default_rng(seed)
    layers = []
    for i, o in zip(widths[:-1], widths[1:]):
        k = gain / np.sqrt(i)
        layers.append((rng.uniform(-k, k, (o, i)).astype(np.float32), rng.uniform(-k, k, o).astype(np.float32)))
    return {"layers": layers, "activation": activation, "taps": tuple(taps), "err_scale": err_scale, "vel_scale": vel_scale,
            "out_scale": out_scale}


def pad_net(net, P):
    """The same net with every hidden width zero-padded to P and the inputs to 8 (what the kernel is handed)."""
    layers, out = net["layers"], []
    for l, (W, b) in enumerate(layers):
        o = W.shape[0] if l == len(layers) - 1 else P
        i = P if (l > 0 or len(layers) == 1) else 8
        Wp, bp = np.zeros((o, i), np.float32), np.zeros(o, np.float32)
        Wp[:W.shape[0], :W.shape[1]], bp[:b.shape[0]] = W, b
        out.append((Wp, bp))
    return dict(net, layers=out)


def activate(x, name):
    if name == "softsign":
        return x / (x.dtype.type(1.0) + np.abs(x))
    if name == "relu":
        return np.where(x > 0, x, x.dtype.type(0.0))
    if name == "tanh":
        return np.tanh(x)
    if name == "elu":
        return np.where(x > 0, x, np.expm1(np.minimum(x, x.dtype.type(0.0))))
    raise ValueError(name)


def forward(net, x, T):
    """Step 5's layers on x (rows, inputs): acc = b_j, then for k ascending acc = acc + (w_jk h_k)."""
    h = x
    for l, (W, b) in enumerate(net["layers"]):
        W, b = W.astype(T), b.astype(T)
        acc = np.broadcast_to(b, (h.shape[0], b.shape[0])).copy()
        for k in range(h.shape[1]):                                # inputs beyond W's columns do not exist in the unpadded net
            if k < W.shape[1]:
                acc = acc + (W[None, :, k] * h[:, k:k + 1])
        h = acc if l == len(net["layers"]) - 1 else activate(acc, net["activation"])
    return h[:, 0]


def _shift(col, reset, fill, v):
    """Steps 1 and 2 on a history (n, S, nd), in place."""
    if reset is not None:
        r = np.asarray(reset).astype(bool)
        col[r] = fill[r][:, None, :] if isinstance(fill, np.ndarray) else fill
    for k in range(col.shape[1] - 1, 0, -1):
        col[:, k] = col[:, k - 1]
    col[:, 0] = v


def step(T, st, target, q, qd, kp=None, kd=None, delay=0, strength=None, saturation=None, velocity_limit=None, effort_limit=None,
         reset=None, net=None):
    """One call in dtype T on a state of dtype T.  target, q, qd (n, nd); kp, kd (nd) or (n, nd); delay an int or (n) ints;
    strength (n, nd); saturation, velocity_limit, effort_limit (nd); reset (n).  Returns a dict: efforts, applied, and what the
    tests count the branches with: pre (the torque before step 7), hi, lo, cap."""
    c = lambda a: None if a is None else np.asarray(a).astype(T)
    t, q, qd = c(target), c(q), c(qd)
    n, nd = t.shape
    L = st["cmd"].shape[1]
    # 1, 2
    _shift(st["cmd"], reset, t, t)
    # 3
    D = np.clip(np.asarray(delay, np.int64), 0, L - 1) if np.ndim(delay) else np.full(n, int(delay), np.int64)
    assert ((D >= 0) & (D < L)).all()
    a = np.take_along_axis(st["cmd"], D[:, None, None].repeat(nd, 2), 1)[:, 0]
    # 4
    err = a - q
    # 5
    if net is None:
        tau = (c(kp) * err) - (c(kd) * qd)
    else:
        _shift(st["err"], reset, T(0.0), err)
        _shift(st["vel"], reset, T(0.0), qd)
        taps = list(net["taps"])
        x = np.concatenate([T(net["err_scale"]) * st["err"][:, taps], T(net["vel_scale"]) * st["vel"][:, taps]], 1)   # (n, 2T, nd)
        x = x.transpose(0, 2, 1).reshape(n * nd, 2 * len(taps))
        tau = (T(net["out_scale"]) * forward(net, x, T)).reshape(n, nd)
    # 6
    if strength is not None:
        tau = tau * c(strength)
    pre = tau
    # 7
    out = {"applied": a, "pre": pre}
    lim = None if effort_limit is None else c(effort_limit)
    if saturation is not None and velocity_limit is not None:
        cap = np.full(nd, np.inf, T) if lim is None else np.where(lim > 0, lim, T(np.inf)).astype(T)
        sat = c(saturation)
        r = qd / c(velocity_limit)
        hi = np.minimum(np.maximum(sat * (T(1.0) - r), T(0.0)), cap)
        lo = np.maximum(np.minimum(sat * (T(-1.0) - r), T(0.0)), -cap)
        tau = np.maximum(np.minimum(tau, hi), lo)
        out.update(hi=hi, lo=lo, cap=np.broadcast_to(cap, hi.shape))
    elif lim is not None:
        clamped = np.maximum(np.minimum(tau, lim), -lim)
        tau = np.where(lim > 0, clamped, tau)
    # 8
    out["efforts"] = tau.astype(T)
    return out


def step32(st, *a, **kw):
    return step(np.float32, st, *a, **kw)


def step64(st, *a, **kw):
    return step(np.float64, st, *a, **kw)


def bound(net, x, strength=None):
    """Per row of x (rows, 2T) float64 (the network's inputs as step64 forms them): a bound on |float32 torque - float64 torque|
    after step 6, from the actual weights.  An input carries 3 u |x| (the subtraction a - q, the scale, and a history slot
    stored in float32); a layer of K inputs maps an error e to (K + 1) u (|b| + |W| |h|) + |W| e; an activation (all four are
    1-Lipschitz) adds 4 u |h|; out_scale and the strength one rounding each.  Steps 7's min / max are 1-Lipschitz."""
    h = np.asarray(x, np.float64)
    e = 3.0 * U * np.abs(h)
    for l, (W, b) in enumerate(net["layers"]):
        W, b = W.astype(np.float64), b.astype(np.float64)
        K = W.shape[1]
        e = (K + 1) * U * (np.abs(b)[None] + np.abs(h) @ np.abs(W).T) + e @ np.abs(W).T
        h = h @ W.T + b[None]
        if l < len(net["layers"]) - 1:
            h = activate(h, net["activation"])
            e = e + 4.0 * U * np.abs(h)
    s = abs(float(net["out_scale"]))
    y, e = s * np.abs(h[:, 0]), s * e[:, 0]
    e = e + U * y
    if strength is not None:
        g = np.abs(np.asarray(strength, np.float64)).reshape(-1)
        e = g * e + U * g * y
    return e


def seeded_call(rng, n, nd, sigma_q=0.4, sigma_qd=8.0):
    """One call's fresh inputs: target and q around the A1's stance, qd ~ N(0, sigma_qd^2)."""
    return {"target": rng.normal(0.0, sigma_q, (n, nd)).astype(np.float32), "q": rng.normal(0.0, sigma_q, (n, nd)).astype(np.float32),
            "qd": rng.normal(0.0, sigma_qd, (n, nd)).astype(np.float32)}
