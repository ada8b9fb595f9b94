"""A lane's row of the response matrix W stays in registers through the sweeps (csrc/shf_chain_hard.h, H3, KC = 8).

The fused chain-mapped A1 step reads its blocks (l, 0..7) of W once behind H2b; the eight unrolled visits of a sweep then
touch no LDS: between the first and the last DPP row broadcast of the kernel (the sweep's code) there is no ds_read.  The
row costs registers, so the same forms are held to their budget: at most 256 VGPRs (AGPRs included), no scratch -- two waves
per SIMD.  Checked on the gfx950 machine code and the resource report of the built library; no GPU needed."""
import json
import os
import re
import subprocess

import pytest

from shifu_amd import build

OBJ = os.path.join(build.HERE, "build", "libshifu_amd.so.obj", "shf_a1_chain.o")     # the unit that holds the chain-mapped solve
# the forms that hold all eight columns: <TW, SELF> of both solvers (bench.py: default, --solver pgs, --workload trimesh, --self-collision)
FULL_ROW = [f"_Z14k_a1_chain_{s}ILb{tw}ELb{sc}EEv6A1Args" for s in ("tgs", "pgs") for tw in (0, 1) for sc in (0, 1)]
# every fused form of the KC = 8 solve
FUSED = FULL_ROW
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


@pytest.fixture(scope="module")
def resources():
    if not os.path.exists(build.LIB) or not os.path.exists(build.RESOURCES):
        pytest.skip("the built library's resource report is not here")
    with open(build.RESOURCES) as f:
        return json.load(f)


@pytest.mark.parametrize("name", FULL_ROW)
def test_no_lds_read_inside_the_sweep(disassembly, name):
    assert name in disassembly, f"{name} is not in the unit"
    ins = disassembly[name]
    at = [i for i, x in enumerate(ins) if BCAST.search(x)]
    assert {int(BCAST.search(ins[i]).group(1)) for i in at} == set(range(8)), f"{name}: not one visit per contact 0..7"
    sweep = ins[at[0]:at[-1] + 1]
    reads = [x for x in sweep if x.startswith("ds_read")]
    assert not reads, f"{name}: {len(reads)} LDS reads between the first and the last visit of the sweep: {reads[:3]}"


@pytest.mark.parametrize("name", FUSED)
def test_fused_forms_keep_two_waves_without_scratch(resources, name):
    assert name in resources, f"{name} is not in the resource report"
    r = resources[name]
    assert r["scratch"] == 0, f"{name}: {r['scratch']} B of scratch"
    assert r["vgprs"] + r.get("agprs", 0) <= 256, f"{name}: {r['vgprs']} VGPRs + {r.get('agprs', 0)} AGPRs"
