"""The selection at the contact cap on its own (csrc/shf_chain_hard.h: hard_cap_select<32, 3, true>, the function the fused A1 step
calls, through shf_cap_select_test) against a stable sort by (gap, position) that keeps the first kmax.

Per env: 88 sample-point slots in slot order, then 32 self-contact entries -- position = index in that row of 120.  The gap is
compared as a float (-0.0 ties with +0.0).  Two envs share a wavefront, so every case has n = 2 .. 4 envs: one or two wavefronts,
the last of them half empty when n is odd.  All cases go to the GPU in one upload; each is a launch of its own."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NS, ROW = 88, 120


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


def _env(entries, kmax):
    """entries: (position, gap) of the candidates -> (gaps, flags, kmax).  Entries that are no candidates carry a gap that would win
    every comparison: the selection must not look at them."""
    g = np.full(ROW, -1.0e30, np.float32)
    f = np.zeros(ROW, np.uint8)
    for p, v in entries:
        assert 0 <= p < ROW and not f[p]
        g[p], f[p] = v, 1
    return g, f, kmax


def _reference(g, f, kmax):
    idx = np.nonzero(f)[0]
    order = idx[np.argsort(g[idx], kind="stable")]          # (-0.0 == +0.0 for the sort's comparisons; equal gaps stay in position order)
    kept = np.zeros(ROW, np.uint8)
    kept[order[:kmax]] = 1
    return kept, order


def _straddles(env):
    """the gap of the last kept candidate equals that of the first dropped one"""
    g, f, kmax = env
    _, order = _reference(g, f, kmax)
    return len(order) > kmax and g[order[kmax - 1]] == g[order[kmax]]


def _run(cases):
    """cases: lists of envs (2 .. 4 each).  Returns per case (got, want), both (n, 120)."""
    from shifu_amd import _lib
    _need_gpu()
    envs = [e for c in cases for e in c]
    gaps = torch.from_numpy(np.stack([e[0] for e in envs])).cuda()
    flags = torch.from_numpy(np.stack([e[1] for e in envs])).cuda()
    kmax = torch.tensor([e[2] for e in envs], dtype=torch.int32).cuda()
    kept = torch.full((len(envs), ROW), 7, dtype=torch.uint8, device="cuda")
    at = 0
    for c in cases:
        assert 2 <= len(c) <= 4
        _lib.check(_lib.lib().shf_cap_select_test(len(c), C.c_void_p(gaps.data_ptr() + at * ROW * 4), C.c_void_p(flags.data_ptr() + at * ROW),
                                                  C.c_void_p(kmax.data_ptr() + at * 4), C.c_void_p(kept.data_ptr() + at * ROW), None))
        at += len(c)
    torch.cuda.synchronize()
    got = kept.cpu().numpy()
    out, at = [], 0
    for c in cases:
        want = np.stack([_reference(*e)[0] for e in c])
        out.append((got[at:at + len(c)], want))
        at += len(c)
    return out


def _check(cases, names=None):
    for i, (got, want) in enumerate(_run(cases)):
        bad = np.argwhere(got != want)
        assert len(bad) == 0, (names[i] if names else i, bad[:6].tolist(), [int(e[2]) for e in cases[i]])


def _spread(count, gaps=None, first=0, step=5):
    """count candidates at positions first, first + step, .. (slots and self entries alike) with distinct gaps unless given"""
    pos = [(first + step * i) % ROW for i in range(count)]
    assert len(set(pos)) == count
    gaps = gaps if gaps is not None else [0.001 * ((7 * i) % count) - 0.004 for i in range(count)]
    return list(zip(pos, gaps))


def test_excess_of_one_of_kmax_and_beyond():
    filler = _env(_spread(5), 8)
    cases, names = [], []
    for kmax in (8, 3, 1, 12):
        for total in (kmax + 1, 2 * kmax, 2 * kmax + 1, 3 * kmax + 6):      # excess 1, = kmax, > kmax (keeps the smallest instead)
            total = min(total, 60)
            cases.append([_env(_spread(total, first=3, step=2), kmax), filler])
            cases.append([filler, _env(_spread(total, first=1, step=1), kmax), _env(_spread(total, first=30, step=7), kmax)])
            names += [f"kmax {kmax} total {total} env 0", f"kmax {kmax} total {total} envs 1, 2"]
    _check(cases, names)


def test_the_two_envs_of_a_wavefront_differ():
    over, under, none = _env(_spread(13), 8), _env(_spread(6, first=2), 8), _env([], 8)
    big = _env(_spread(30, step=4), 8)                        # excess 22 > kmax beside an excess of 5
    _check([[over, under], [under, over], [over, none], [none, over], [over, big], [big, over], [over, none, none, big], [none, none]])


def test_ties_at_the_cut():
    t = 0.0025
    cases = {
        # five below the tie, then four equal gaps of which three are kept (kmax 8): inside row 0, across rows 0 and 1, across
        # rows 1 and 2 of the same lanes, between a slot and a self entry, among self entries
        "within a row": _env([(i, -0.01 - 0.0001 * i) for i in range(40, 45)] + [(p, t) for p in (3, 9, 17, 30)] + [(50, 0.01)], 8),
        "across two rows": _env([(i, -0.01 - 0.0001 * i) for i in range(40, 45)] + [(p, t) for p in (5, 20, 37, 52)] + [(60, 0.01)], 8),
        "same lane, rows 1 and 2": _env([(i, -0.01) for i in range(5)] + [(p, t) for p in (33, 34, 65, 66)], 8),
        "slot and self entry": _env([(i, -0.01) for i in range(5)] + [(p, t) for p in (10, 70, 87, 88)] + [(100, 0.02)], 8),
        "self entries": _env([(i, -0.01) for i in range(5)] + [(p, t) for p in (90, 95, 96, 119)], 8),
        "all gaps equal, excess 3": _env([(p, t) for p in range(4, ROW, 11)], 8),
        "all gaps equal": _env([(p, t) for p in range(0, ROW, 7)], 8),
        "all gaps equal, excess beyond kmax": _env([(p, t) for p in range(0, ROW, 3)], 8),
        "all gaps equal, kmax 1": _env([(p, t) for p in (31, 32, 64, 88)], 1),
        # -0.0f against +0.0f: equal gaps, so position alone decides, whichever sign sits first
        "-0 then +0": _env([(2, -0.5), (40, -0.0), (41, 0.0), (42, -0.0), (90, 0.0)], 3),
        "+0 then -0": _env([(2, -0.5), (40, 0.0), (41, -0.0), (89, -0.0), (90, 0.0)], 3),
        "-0 in the keep-smallest branch": _env([(p, -0.0 if p % 2 else 0.0) for p in range(20, 60)] + [(3, 1.0)], 8),
    }
    for name, env in cases.items():
        assert _straddles(env), name
    neg = cases["-0 then +0"]
    assert np.signbit(neg[0][40]) and not np.signbit(neg[0][41])
    names = list(cases)
    filler = _env(_spread(11, first=1), 8)
    _check([[cases[k], filler] for k in names] + [[filler, cases[k], cases[k]] for k in names], names + names)


def test_candidates_in_one_row_only():
    row2 = _env([(64 + i, 0.001 * ((5 * i) % 24)) for i in range(24)], 8)              # all 24 slots of row 2
    row2_few = _env([(64 + 2 * i, 0.01 - 0.001 * i) for i in range(10)], 8)
    selfs = _env([(NS + i, 0.001 * ((11 * i) % 32)) for i in range(32)], 8)             # all 32 self entries, none else
    selfs_few = _env([(NS + 3 * i, 0.01 - 0.001 * i) for i in range(9)], 8)
    _check([[row2, selfs], [selfs, row2], [row2_few, selfs_few], [selfs_few, row2_few, row2, selfs]])


def _random_cases():
    rng = np.random.default_rng(12)
    values = np.array([-0.01, -0.0, 0.0, 0.004, 0.004000001, 0.01, 0.02], np.float32)
    cases, tied, keepmode = [], 0, 0
    for _ in range(300):
        c = []
        for _ in range(int(rng.integers(2, 5))):
            kmax = int(rng.choice([1, 3, 8, 8, 8, 12, 16]))
            count = int(rng.choice([0, rng.integers(1, kmax + 1), rng.integers(kmax + 1, 2 * kmax + 2), rng.integers(kmax + 1, 50)]))
            pos = rng.choice(ROW, size=count, replace=False)
            env = _env([(int(p), float(v)) for p, v in zip(pos, rng.choice(values, size=count))], kmax)
            tied += _straddles(env)
            keepmode += count > 2 * kmax
            c.append(env)
        cases.append(c)
    return cases, tied, keepmode


def test_random_cases_with_many_ties():
    cases, tied, keepmode = _random_cases()
    assert len(cases) == 300 and tied > 100 and keepmode > 50
    _check(cases)
