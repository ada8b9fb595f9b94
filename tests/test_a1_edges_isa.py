"""The edges of the chain-mapped fused A1 step -- the code before and after its sub-step loop (csrc/shf_chain.h:
a1_chain_step_body; csrc/shf_task.h: a1_post_step) -- keep their shape in the gfx950 machine code.

Before the block's first barrier every global load is issued before the first wait on the vector-memory counter: the step
counter, the env's state and action, the task parameters and the three blocks of the model are one round trip, not six
one behind another.  The first such wait leaves loads outstanding (it waits for the step counter, the oldest load, alone:
the random actions' Philox rounds run under the others).  After the sub-step loop nothing divides by a run-time integer:
the chain kernels pass their dimensions as constants, and the history's (dof, slot) indices are advanced, not divided out.
Order of loads and waits and instruction counts only; checked on the built library, no GPU needed."""
import os
import re
import subprocess

import pytest

from shifu_amd import build

OBJ = os.path.join(build.HERE, "build", "libshifu_amd.so.obj", "shf_a1_chain.o")     # the unit that holds the chain-mapped step
FAMILIES = ("_Z14k_a1_chain_tgsI", "_Z14k_a1_chain_pgsI")
VMCNT = re.compile(r"s_waitcnt\b.*\bvmcnt\((\d+)\)")
BCAST = re.compile(r"row_newbcast:(\d+)")
TARGET = re.compile(r"<[^>+]+\+0x([0-9a-f]+)>")


def _tool(name):
    try:
        return build._llvm_tool(name)
    except RuntimeError:
        return None


@pytest.fixture(scope="module")
def disassembly(tmp_path_factory):
    """kernel symbol -> [(address, instruction)], from the gfx950 code object of the unit."""
    tools = {n: _tool(n) for n in ("llvm-objcopy", "clang-offload-bundler", "llvm-objdump")}
    if not os.path.exists(build.LIB) or not os.path.exists(OBJ) or None in tools.values():
        pytest.skip("the built library or the ROCm LLVM tools are not here")
    td = tmp_path_factory.mktemp("isa")
    fat, co = str(td / "fat.bin"), str(td / "k.co")
    subprocess.run([tools["llvm-objcopy"], "-O", "binary", "--only-section=.hip_fatbin", OBJ, fat], check=True, capture_output=True)
    subprocess.run([tools["clang-offload-bundler"], "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--unbundle",
                    "--input=" + fat, "--output=" + co], check=True, capture_output=True)
    text = subprocess.run([tools["llvm-objdump"], "-d", "--mcpu=gfx950", co], check=True, capture_output=True, text=True).stdout
    out, cur, base = {}, None, 0
    for line in text.splitlines():
        m = re.match(r"^([0-9a-f]+) <([^>]+)>:", line)
        if m:
            cur, base = out.setdefault(m.group(2), []), int(m.group(1), 16)
        elif cur is not None and line.startswith("\t") and "//" in line:
            ins, note = line.split("//", 1)
            m = TARGET.search(note)
            cur.append((int(note.split(":")[0].strip(), 16) - base, ins.strip() + (" " + m.group(0) if m else "")))
    return out


def _kernels(dis, family):
    ks = {n: v for n, v in dis.items() if n.startswith(family)}
    assert len(ks) == 4, f"{family}: expected the four TW / SELF forms, found {sorted(ks)}"
    return ks


def _epilogue(code):
    """The instructions behind the sub-step loop: behind the last backward branch that jumps over the contact sweeps to a place
    behind the block's first barrier (the sweeps' DPP broadcasts mark them; the outermost loop around them is the sub-step loop;
    a block of the prologue laid out at the kernel's end jumps back in front of the barrier)."""
    sweeps = [a for a, x in code if BCAST.search(x)]
    barrier = next(a for a, x in code if x.startswith("s_barrier"))
    back = [i for i, (a, x) in enumerate(code) if x.startswith(("s_cbranch", "s_branch")) and a > sweeps[-1]
            for m in [TARGET.search(x)] if m and barrier < int(m.group(1), 16) < sweeps[0]]
    assert back, "no loop around the sweeps"
    return [x for _, x in code[back[-1] + 1:]]


@pytest.mark.parametrize("family", FAMILIES)
def test_prologue_issues_every_load_before_its_first_wait(disassembly, family):
    for name, code in _kernels(disassembly, family).items():
        ins = [x for _, x in code]
        pro = ins[:next(i for i, x in enumerate(ins) if x.startswith("s_barrier"))]
        loads = [i for i, x in enumerate(pro) if x.startswith("global_load")]
        waits = [(i, int(m.group(1))) for i, x in enumerate(pro) for m in [VMCNT.search(x)] if m]
        assert len(loads) >= 6, f"{name}: {len(loads)} global loads before the first barrier (counter, state, action, parameters, model)"
        assert waits, f"{name}: no wait on the vector-memory counter before the first barrier"
        late = [pro[i] for i in loads if i > waits[0][0]]
        assert not late, f"{name}: global loads behind a vmcnt wait in the prologue: {late[:3]}"
        assert waits[0][1] > 0, f"{name}: the first wait drains every load ({pro[waits[0][0]]}); it is to wait for the step counter alone"


def test_epilogue_has_no_run_time_integer_division(disassembly):
    (name, code), = [(n, v) for n, v in disassembly.items() if n.startswith("_Z14k_a1_chain_tgsILb0ELb0EE")]
    tail = _epilogue(code)
    assert 1000 < len(tail) < len(code) // 2, f"{name}: {len(tail)} of {len(code)} instructions behind the sub-step loop"
    bad = [x for x in tail if x.startswith("v_rcp_iflag_f32")]
    assert not bad, f"{name}: {len(bad)} v_rcp_iflag_f32 behind the sub-step loop (an integer division by a run-time value)"
