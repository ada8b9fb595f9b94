"""The contact sweep of the velocity-level solve at eight constraints per env stays unrolled (csrc/shf_chain_hard.h, H3).

Each of the eight visits has its contact index as a constant: the change of the impulse reaches the owner lanes by a DPP
row broadcast (row_newbcast:c), and no v_readlane takes its lane from an SGPR there.  A compiler that rolled the visits
back into a loop would need a lane index in a register again.  Checked on the gfx950 machine code of the built library;
no GPU needed."""
import os
import re
import subprocess

import pytest

from shifu_amd import build

OBJ = os.path.join(build.HERE, "build", "libshifu_amd.so.obj", "shf_a1_chain.o")     # the unit that holds the chain-mapped solve
FAMILIES = ("_Z14k_a1_chain_tgsI", "_Z14k_a1_chain_pgsI", "_Z20k_sim_step_chain_tgsI", "_Z20k_sim_step_chain_pgsI")
SGPR_LANE_READ = re.compile(r"v_readlane_b32\s+s\d+,\s*v\d+,\s*s\d+\b")
BCAST = re.compile(r"row_newbcast:(\d+)")


def _tool(name):
    try:
        return build._llvm_tool(name)
    except RuntimeError:
        return None


@pytest.fixture(scope="module")
def disassembly(tmp_path_factory):
    """kernel symbol -> its instructions, from the gfx950 code object of the unit."""
    tools = {n: _tool(n) for n in ("llvm-objcopy", "clang-offload-bundler", "llvm-objdump")}
    if not os.path.exists(build.LIB) or not os.path.exists(OBJ) or None in tools.values():
        pytest.skip("the built library or the ROCm LLVM tools are not here")
    td = tmp_path_factory.mktemp("isa")
    fat, co = str(td / "fat.bin"), str(td / "k.co")
    subprocess.run([tools["llvm-objcopy"], "-O", "binary", "--only-section=.hip_fatbin", OBJ, fat], check=True, capture_output=True)
    subprocess.run([tools["clang-offload-bundler"], "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--unbundle",
                    "--input=" + fat, "--output=" + co], check=True, capture_output=True)
    text = subprocess.run([tools["llvm-objdump"], "-d", "--mcpu=gfx950", co], check=True, capture_output=True, text=True).stdout
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <([^>]+)>:", line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and line.startswith("\t"):
            cur.append(line.split("//")[0].strip())
    return out


def _kernels(dis, family):
    ks = {n: v for n, v in dis.items() if n.startswith(family)}
    assert len(ks) == 4, f"{family}: expected the four TW / SELF forms, found {sorted(ks)}"
    return ks


@pytest.mark.parametrize("family", FAMILIES)
def test_every_visit_broadcasts_by_dpp(disassembly, family):
    for name, ins in _kernels(disassembly, family).items():
        lanes = {int(m.group(1)) for x in ins for m in [BCAST.search(x)] if m}
        assert lanes == set(range(8)), f"{name}: row_newbcast lanes {sorted(lanes)}, expected one visit per contact 0..7"


@pytest.mark.parametrize("family", FAMILIES)
def test_no_lane_index_in_an_sgpr_inside_the_sweep(disassembly, family):
    for name, ins in _kernels(disassembly, family).items():
        at = [i for i, x in enumerate(ins) if BCAST.search(x)]
        sweep = ins[at[0]:at[-1] + 1]
        bad = [x for x in sweep if SGPR_LANE_READ.search(x)]
        assert not bad, f"{name}: the unrolled sweep reads lanes by an SGPR index: {bad[:3]}"
