"""The issue slots of the KC = 8 contact sweep that compute nothing (csrc/shf_chain_hard.h, SLOTS; profiles/r24_sweep_slots.md).

Between the first and the last DPP row broadcast of each fused chain-mapped A1 kernel that took the change -- a little over seven
of the eight unrolled visits -- there is no s_waitcnt (the lane's row of W is resident before the sweeps), no canonicalising
v_max_f32 v, v, v (the sliding step's floor is one v_max_f32), at most two branches per contact (the skip rule and the sliding
step; no count test), and no more instructions than the change left there.  Checked on the gfx950 code object of the built
library; no GPU needed."""
import re

import pytest

from tests.test_sweep_wreg_isa import BCAST, FUSED, disassembly      # noqa: F401  (the fixture)

# the fused forms behind SLOTS: all eight (none had to stay on the parent's path for its registers)
TOOK = FUSED
# instructions from the first to the last row_newbcast: a build of the parent commit, and what the change left
SPAN_PARENT = {"tgs": 564, "pgs": 554}
SPAN_NOW = {"tgs": 505, "pgs": 519}
DRIFT = 16
SAME_MAX = re.compile(r"^v_max_f32(_e32|_e64)?\s+(v\d+),\s*(v\d+),\s*(v\d+)$")
BRANCH = ("s_cbranch", "s_branch")


def _sweep(disassembly, name):
    assert name in disassembly, f"{name} is not in the unit"
    ins = disassembly[name]
    at = [i for i, x in enumerate(ins) if BCAST.search(x)]
    assert {int(BCAST.search(ins[i]).group(1)) for i in at} == set(range(8)), f"{name}: not one visit per contact 0..7"
    return ins[at[0]:at[-1] + 1]


@pytest.mark.parametrize("name", TOOK)
def test_no_wait_inside_the_sweep(disassembly, name):
    waits = [x for x in _sweep(disassembly, name) if x.startswith("s_waitcnt")]
    assert not waits, f"{name}: {len(waits)} s_waitcnt between the first and the last visit of the sweep: {waits[:3]}"


@pytest.mark.parametrize("name", TOOK)
def test_no_canonicalising_max_inside_the_sweep(disassembly, name):
    same = [x for x in _sweep(disassembly, name) if (m := SAME_MAX.match(x)) and m.group(2) == m.group(3) == m.group(4)]
    assert not same, f"{name}: {len(same)} v_max_f32 of a register with itself between the first and the last visit: {same[:3]}"


@pytest.mark.parametrize("name", TOOK)
def test_two_branches_per_contact_at_the_most(disassembly, name):
    branches = [x for x in _sweep(disassembly, name) if x.startswith(BRANCH)]
    assert len(branches) <= 2 * 8, f"{name}: {len(branches)} branches between the first and the last visit of eight contacts"


@pytest.mark.parametrize("name", TOOK)
def test_the_sweep_is_no_longer_than_the_change_left_it(disassembly, name):
    sweep = _sweep(disassembly, name)
    solver = "tgs" if "_tgs" in name else "pgs"
    assert SPAN_NOW[solver] + DRIFT < SPAN_PARENT[solver] - DRIFT      # the saving is more than the drift allowed on both sides
    assert len(sweep) <= SPAN_NOW[solver] + DRIFT, f"{name}: {len(sweep)} instructions from the first to the last visit (parent {SPAN_PARENT[solver]})"
