"""The shape of one visit of the KC = 8 contact sweep in the machine code (csrc/shf_chain_hard.h, visit8; profiles/r10_sweep_visit.md).

Between the first and the last DPP row broadcast of each fused chain-mapped A1 kernel -- the eight unrolled visits of a sweep --
there is no exec-masked block (the sliding step computes its scale on every lane and selects), no register-to-register copy (the
committing lanes take impulse and velocity in place), three broadcasts per contact, and no more instructions than the change left
there.  Checked on the gfx950 code object of the built library; no GPU needed."""
import re

import pytest

from tests.test_sweep_wreg_isa import BCAST, FUSED, disassembly      # noqa: F401  (the fixture)

# instructions from the first to the last row_newbcast: the parent commit, and what the change left (profiles/r10_sweep_visit.md,
# "ISA of the sweep"); the bound is what was achieved plus 16 for compiler drift
SPAN_PARENT = {"tgs": 607, "pgs": 617}
SPAN_NOW = {"tgs": 565, "pgs": 554}
DRIFT = 16
COPY = re.compile(r"^v_mov_b32(_e32|_e64)?\s+v\d+,\s*v\d+$")


def _sweep(disassembly, name):
    assert name in disassembly, f"{name} is not in the unit"
    ins = disassembly[name]
    at = [i for i, x in enumerate(ins) if BCAST.search(x)]
    assert at, f"{name}: no row_newbcast"
    return ins, at, ins[at[0]:at[-1] + 1]


@pytest.mark.parametrize("name", FUSED)
def test_no_exec_masked_block_and_no_copies_inside_the_sweep(disassembly, name):
    ins, at, sweep = _sweep(disassembly, name)
    masked = [x for x in sweep if x.startswith("s_and_saveexec")]
    assert not masked, f"{name}: {len(masked)} exec-masked blocks between the first and the last visit of the sweep"
    copies = [x for x in sweep if COPY.match(x)]
    assert not copies, f"{name}: {len(copies)} register-to-register copies between the first and the last visit: {copies[:3]}"


@pytest.mark.parametrize("name", FUSED)
def test_three_broadcasts_per_contact(disassembly, name):
    ins, at, sweep = _sweep(disassembly, name)
    per = {}
    for i in at:
        c = int(BCAST.search(ins[i]).group(1))
        per[c] = per.get(c, 0) + 1
    assert per == {c: 3 for c in range(8)}, f"{name}: row_newbcast per contact {per}"


@pytest.mark.parametrize("name", FUSED)
def test_the_sweep_is_no_longer_than_the_change_left_it(disassembly, name):
    ins, at, sweep = _sweep(disassembly, name)
    solver = "tgs" if "_tgs" in name else "pgs"
    assert SPAN_NOW[solver] + DRIFT < SPAN_PARENT[solver] - DRIFT      # the saving is more than the drift allowed on both sides
    assert len(sweep) <= SPAN_NOW[solver] + DRIFT, f"{name}: {len(sweep)} instructions from the first to the last visit (parent {SPAN_PARENT[solver]})"
