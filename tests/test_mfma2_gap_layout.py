"""Layout of the exact-fp32 GRU step around its barrier, read from the disassembly (CPU; compiles gru_mfma2.hip as
tools/check_barrier_asm.py does, for libntm.so and with -DNTM_LAB for libntm_lab.so).

The wave issues in order and the matrix pipe takes one v_mfma_f32_16x16x4_f32 per 32 cycles, so whatever sits between two
MFMAs is free only while it fits the ~24 issue cycles an MFMA leaves over (DESIGN.md, K1 cycle budget).  For every
non-diagnostic ENGINE 0 instantiation, at every step barrier (`s_waitcnt lgkmcnt(1); s_barrier`):
  * no LDS instruction sits between the barrier and the next v_mfma (the wait and the barrier have that gap to themselves);
  * no gap between two consecutive v_mfma of the step's block holds more than one ds_read_b128;
  * the step's three reads of the other quarters of h all precede the 13th MFMA behind the barrier (the first that needs one).
The MFMA-richest loop (the whole-tile loop with its unrolled and compile-time housekeeping steps) must hold at least ten
such barriers; the copies outside it (the run-time tail) are held to the same layout."""
import os
import re
import subprocess

import pytest

from helpers import ROOT

SRC = os.path.join(ROOT, "neural-tape-modeling_amd", "csrc", "gru_mfma2.hip")
WINDOW = 36        # MFMAs behind a barrier that belong to its step whatever NTM2_NB is (48 - 3 NB >= 39)


@pytest.fixture(scope="module")
def disassembly(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("mfma2_asm")
    procs = {}
    for tag, defines in (("product", []), ("lab", ["-DNTM_LAB"])):       # side by side: ~12 s each
        out = str(tmp / (tag + ".s"))
        procs[tag] = (out, subprocess.Popen(
            ["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"), "-Wno-unused-function",
             "-mllvm", "-amdgpu-mfma-vgpr-form", "-S", "--cuda-device-only", "-o", out, SRC] + defines, stderr=subprocess.DEVNULL))
    texts = {}
    for tag, (out, p) in procs.items():
        assert p.wait() == 0, f"hipcc failed on the {tag} build"
        with open(out) as f:
            texts[tag] = f.read()
    return texts


def _engine0_products(text):
    """[(mangled name, [instruction or 'LABEL name'])] of the non-diagnostic ENGINE 0 instantiations."""
    out = []
    for name, body in re.findall(r"^(_ZN3ntm16gru_mfma2_kernel\w+):[^\n]*\n(.*?)\n\s*\.amdhsa_kernel", text, flags=re.S | re.M):
        m = re.match(r"_ZN3ntm16gru_mfma2_kernelILb1ELb(\d)ELi(\d+)ELi(\d)ELi(\d+)E((?:Lb\dE)*)EE", name)
        if not m or m.group(1) != "0" or m.group(2) != "0" or m.group(3) != "0":
            continue                                   # STAMP / ablation builds; the split engines keep their own order
        ins = []
        for ln in body.splitlines():
            lab = re.match(r"\s*(\.LBB\w+):", ln)
            t = ln.split(";")[0].strip()
            if lab:
                ins.append("LABEL " + lab.group(1))
            elif t:
                ins.append(t)
        out.append((name, ins))
    return out


def _hot_loop(ins):
    """(first, last) instruction index of the loop that holds the most MFMAs."""
    labels = {t.split()[1]: i for i, t in enumerate(ins) if t.startswith("LABEL ")}
    best = (0, 0, 0)
    for i, t in enumerate(ins):
        m = re.match(r"s_c?branch\w*\s+(\.LBB\w+)", t)
        if m and labels.get(m.group(1), i + 1) <= i:
            a = labels[m.group(1)]
            best = max(best, (sum(1 for u in ins[a:i + 1] if u.startswith("v_mfma")), a, i))
    return best[1], best[2]


@pytest.mark.parametrize("build", ["product", "lab"])
def test_one_lds_operation_per_mfma_gap_behind_the_step_barrier(disassembly, build):
    kernels = _engine0_products(disassembly[build])
    assert len(kernels) >= (12 if build == "product" else 2), [n for n, _ in kernels]
    for name, ins in kernels:
        a, b = _hot_loop(ins)
        barriers = [i for i, t in enumerate(ins) if t == "s_barrier" and "lgkmcnt(1)" in ins[i - 1]]
        assert sum(1 for i in barriers if a <= i <= b) >= 10, f"{name}: hot loop not found"
        for i in barriers:
            gaps, k = [[]], i + 1                      # gaps[g]: what sits behind the g-th MFMA behind the barrier
            while k < len(ins) and len(gaps) <= WINDOW:
                if ins[k].startswith("v_mfma"):
                    gaps.append([])
                else:
                    gaps[-1].append(ins[k])
                k += 1
            assert len(gaps) == WINDOW + 1, f"{name}: {len(gaps) - 1} MFMAs behind a step barrier"
            where = f"{name}, barrier at instruction {i}"
            assert not [t for t in gaps[0] if t.startswith("ds_")], f"{where}: {gaps[0]} between the barrier and the next MFMA"
            reads = [sum(1 for t in g if t.startswith("ds_read_b128")) for g in gaps[:WINDOW]]
            assert max(reads) <= 1, f"{where}: ds_read_b128 per gap {reads}"
            assert sum(reads[:13]) == 3 and sum(reads) == 3, f"{where}: ds_read_b128 per gap {reads}"
