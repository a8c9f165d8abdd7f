"""CPU guard on the gfx950 ISA of libti_hip.so: the F = 256 message kernels keep no SGPR in the lanes of a VGPR.

painn_edge_nb8.hip (the F = 256 instantiations of painn_edge_kernel, NBK = 16) faulted on the device when hipcc spilled SGPRs into lanes
of a VGPR that stayed live across the kernel (`v_writelane_b32 v255, s4, 0` ... restored with `v_readlane_b32` in front of the address
computations).  build.py compiles that unit with `-mllvm -amdgpu-spill-sgpr-to-vgpr=0`; the compiler then spills SGPRs to
scratch memory instead, which on AMDGPU still passes through the lanes of a temporary VGPR: the VGPR is saved to scratch, the SGPRs are
written into its lanes, it is stored to scratch, and its old contents are loaded back (the reload reads the lanes right after a scratch
load).  So the guard is: in every painn_edge_kernel<16, ...>, each run of lane writes into a VGPR is followed by a scratch store of that
VGPR before anything else reads it, and each run of lane reads from a VGPR comes right after a scratch load into it.  csrc/ has no
hand-written lane instructions, so every one of them is compiler spill code.  The per-kernel lane-instruction counts of the whole
library are printed (run with -s); only the F = 256 message kernels are held to the rule.
"""
import collections
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from conftest import ROOT

LIB = os.path.join(ROOT, "thermodynamic-interpolation_amd", "libti_hip.so")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
GUARDED = re.compile(r"painn_edge_kernel<16,")
LANE_W = re.compile(r"\bv_writelane_b32\s+(v\d+),")
LANE_R = re.compile(r"\bv_readlane_b32\s+s\d+,\s*(v\d+),")
QUIET = re.compile(r"^\s*s_(waitcnt|nop)\b")


def _tool(name):
    for d in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin"), "/opt/rocm/lib/llvm/bin"):
        p = os.path.join(d, name)
        if os.path.exists(p):
            return p
    return shutil.which(name)


def code_objects(lib, tmp):
    """The gfx950 code objects of every translation unit linked into `lib` (one offload bundle per unit in .hip_fatbin)."""
    objcopy, bundler = _tool("llvm-objcopy"), _tool("clang-offload-bundler")
    fat = os.path.join(tmp, "fatbin")
    subprocess.run([objcopy, f"--dump-section=.hip_fatbin={fat}", lib, os.path.join(tmp, "stripped")], check=True, capture_output=True)
    data = open(fat, "rb").read()
    starts = [m.start() for m in re.finditer(re.escape(MAGIC), data)] + [len(data)]
    out = []
    for i in range(len(starts) - 1):
        part, co = os.path.join(tmp, f"bundle{i}"), os.path.join(tmp, f"bundle{i}.co")
        with open(part, "wb") as f:
            f.write(data[starts[i]:starts[i + 1]])
        targets = subprocess.run([bundler, "--list", "--type=o", f"--input={part}"], check=True, capture_output=True, text=True).stdout.split()
        if TARGET in targets:
            subprocess.run([bundler, "--unbundle", "--type=o", f"--targets={TARGET}", f"--input={part}", f"--output={co}"], check=True,
                           capture_output=True)
            out.append(co)
    return out


def kernels(co):
    """{demangled symbol: [instruction lines]} of one code object."""
    asm = subprocess.run([_tool("llvm-objdump"), "-d", "-C", "--no-show-raw-insn", co], check=True, capture_output=True, text=True).stdout
    funcs, cur = {}, None
    for line in asm.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.*)>:$", line)
        if m:
            cur = funcs.setdefault(m.group(1), [])
        elif cur is not None and line.startswith("\t"):
            cur.append(line.split("//")[0].strip())
    return funcs


def lane_spills_outside_scratch(insns):
    """Lane instructions that are not part of an SGPR spill to scratch memory (see the module docstring); [] if all are."""
    bad = []
    for i, ins in enumerate(insns):
        m = LANE_W.search(ins)
        if m:
            v = m.group(1)
            ref = re.compile(rf"\b{v}\b")
            j = i + 1
            while j < len(insns) and (QUIET.match(insns[j]) or LANE_W.search(insns[j]) and LANE_W.search(insns[j]).group(1) == v):
                j += 1
            nxt = insns[j] if j < len(insns) else ""
            if not (nxt.startswith(("scratch_store_dword", "buffer_store_dword")) and ref.search(nxt)):
                bad.append(f"{i}: {ins}  -> next use of {v}: {nxt!r}")
        m = LANE_R.search(ins)
        if m:
            v = m.group(1)
            ref = re.compile(rf"\b{v}\b")
            j = i - 1
            while j >= 0 and (QUIET.match(insns[j]) or LANE_R.search(insns[j]) and LANE_R.search(insns[j]).group(1) == v):
                j -= 1
            prv = insns[j] if j >= 0 else ""
            if not (prv.startswith(("scratch_load_dword", "buffer_load_dword")) and ref.search(prv.split(",")[0])):
                bad.append(f"{i}: {ins}  <- previous def of {v}: {prv!r}")
    return bad


def lane_count(insns):
    return sum(1 for s in insns if LANE_W.search(s) or LANE_R.search(s))


@pytest.fixture(scope="module")
def isa():
    missing = [t for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-objdump") if not _tool(t)]
    if missing:
        pytest.skip(f"ROCm LLVM tools not found: {missing}")
    if not os.path.exists(LIB):
        pytest.skip(f"{LIB} not built (run __graft_entry__.build())")
    with tempfile.TemporaryDirectory() as tmp:
        return [kernels(co) for co in code_objects(LIB, tmp)]


def test_f256_message_kernels_hold_no_sgpr_in_vgpr_lanes(isa):
    guarded = {name: insns for funcs in isa for name, insns in funcs.items() if GUARDED.search(name)}
    # 4 layer positions x 3 precisions x NS 2 / 4, four-wave workgroups (painn_edge_kernel.hpp: configure_edge_nb<8>)
    assert len(guarded) == 24, sorted(guarded)
    report = collections.Counter()
    for funcs in isa:
        for name, insns in funcs.items():
            n = lane_count(insns)
            if n:
                report[name] = n
    print("\nlane instructions per kernel (SGPR spill code):")
    for name, n in sorted(report.items()):
        print(f"  {n:5d}  {name}{'   [guarded: through scratch]' if GUARDED.search(name) else ''}")
    bad = {name: lane_spills_outside_scratch(insns) for name, insns in guarded.items()}
    bad = {k: v for k, v in bad.items() if v}
    assert not bad, "SGPRs held in VGPR lanes (the F = 256 fault pattern, DESIGN.md 3.4):\n" + "\n".join(
        f"{k}: {len(v)} e.g. {v[0]}" for k, v in bad.items())


def test_the_guard_tells_the_two_spill_forms_apart():
    """The rule on hand-written sequences: SGPRs spilled to scratch through a temporary VGPR pass, SGPRs parked in lanes fail."""
    to_scratch = ["scratch_store_dword off, v1, off offset:48", "s_waitcnt lgkmcnt(0)", "v_writelane_b32 v1, s16, 0",
                  "v_writelane_b32 v1, s17, 1", "scratch_store_dword off, v1, off offset:52", "scratch_load_dword v1, off, off offset:48",
                  "s_mov_b32 s2, 0", "scratch_load_dword v1, off, off offset:52", "s_waitcnt vmcnt(0)", "v_readlane_b32 s16, v1, 0",
                  "v_readlane_b32 s17, v1, 1", "scratch_load_dword v1, off, off offset:48"]
    in_lanes = ["v_writelane_b32 v255, s4, 0", "v_writelane_b32 v255, s5, 1", "v_mov_b32 v0, s6", "s_add_u32 s4, s4, 16",
                "v_readlane_b32 s36, v255, 0", "v_readlane_b32 s37, v255, 1", "v_lshl_add_u64 v[2:3], s[36:37], 0, v[4:5]"]
    assert lane_spills_outside_scratch(to_scratch) == []
    assert len(lane_spills_outside_scratch(in_lanes)) == 4
