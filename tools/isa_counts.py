#!/usr/bin/env python3
"""Counts the instructions of the mixed addition (xyzz_madd, csrc/curve.hpp: the bucket update of k_accum_l0) in the
gfx950 ISA: the device code is built with -DBPMI_ISA_PROBE, which adds a probe kernel that runs exactly the main path
of the addition (xyzz_madd_pr + xyzz_madd_finish: the common case, accumulator and addend finite and different)
on operands it loads from memory; every instruction of that kernel is tallied by mnemonic (memory instructions and waits
separately).

    python tools/isa_counts.py                       # prints the JSON object
    python tools/isa_counts.py --write               # also writes profiles/r04_isa_counts.json and the ISA excerpt
    python tools/isa_counts.py --loops [--write]     # the per-entry loops of k_accum_l0<false, true> and of both k_accum_runs instantiations
                                                     # (<true>: dense point fetch), block by block, and what stands in front of the loop
                                                     # (k_accum_runs: the first two entries of a run) counted on its own
                                                     # (--write: profiles/accum_loop_isa_ledger.json)

--loops tallies the whole loop, not only the addition: the loop is the first outermost backward branch whose span holds a whole
mixed addition (>= 900 v_mad_u64_u32); its basic blocks are listed in program order with their instruction, multiply-add and
memory-instruction counts and with how they are entered (a block behind s_cbranch_execz costs nothing only when NO lane of the wave
needs it).  The common path is every block of the loop but the doubling and the rare blocks outlined behind it: what a wave issues
per entry when some lane needs each of the other paths.  What lies behind the loop is the epilogue (k_accum_l0: the wave scan with
its general additions; k_accum_runs: one store).

bench.py reads profiles/r04_isa_counts.json for `alu_roofline.frac_vs_raw_mad` (multiply-adds actually issued per
second against the chip's raw v_mad_u64_u32 rate)."""
import collections
import json
import os
import re
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "python-bulletproofs_amd", "csrc", "bpmi.hip")
INSTR = re.compile(r"^\s+((?:v_|s_|ds_|global_|buffer_|flat_|scratch_)\w+)")


LABEL = re.compile(r"^(\.LBB\d+_\d+):")
BRANCH = re.compile(r"^\s+(s_cbranch_\w+|s_branch)\s+(\.LBB\d+_\d+)")


def loop_tally(kernel):
    """The per-entry loop of an accumulation kernel and what follows it, as basic blocks in program order."""
    blocks, cur, entered = [], None, "falls through"
    for ln in kernel.splitlines():
        m = LABEL.match(ln)
        if m or cur is None:
            cur = {"label": m.group(1) if m else "(entry)", "instructions": 0, "v_mad_u64_u32": 0, "memory_instructions": 0, "entered": entered, "branches": []}
            blocks.append(cur)
            entered = "falls through"
            if m:
                continue
        mm = INSTR.match(ln)
        if not mm:
            continue
        cur["instructions"] += 1
        cur["v_mad_u64_u32"] += 1 if mm.group(1) == "v_mad_u64_u32" else 0
        cur["memory_instructions"] += 1 if mm.group(1).startswith(("global_", "ds_", "buffer_", "flat_", "scratch_")) else 0
        br = BRANCH.match(ln)
        if br:
            cur["branches"].append(br.group(1) + " " + br.group(2))
            entered = "by branch only" if br.group(1) == "s_branch" else "falls through, skipped when " + br.group(1)
    index = {b_["label"]: k for k, b_ in enumerate(blocks)}
    targets = lambda b_: [index[t.split()[1]] for t in b_["branches"] if t.split()[1] in index]
    # loops: [head, last block that branches back to head]; the per-entry loop is the first one that is in no other and holds an addition
    spans = {}
    for k, b_ in enumerate(blocks):
        for t in targets(b_):
            if t <= k:
                spans[t] = max(spans.get(t, k), k)
    mads = lambda lo, hi: sum(b_["v_mad_u64_u32"] for b_ in blocks[lo:hi + 1])
    outer = [(lo, hi) for lo, hi in sorted(spans.items()) if mads(lo, hi) >= 900 and not any(l2 <= lo and hi <= h2 and (l2, h2) != (lo, hi) for l2, h2 in spans.items())]
    lo, hi = outer[0]
    # blocks the compiler laid out behind the loop that jump back into it (rare paths) are the loop's
    end = hi
    for k in range(hi + 1, len(blocks)):
        into = [t for t in targets(blocks[k]) if lo <= t <= hi]
        if not into:
            break
        if blocks[k]["branches"][-1].startswith("s_branch"):
            end = k
    head, body, tail = blocks[:lo], blocks[lo:end + 1], blocks[end + 1:]
    count = lambda bs, key: sum(b_[key] for b_ in bs)
    # the rare paths of the mixed addition: the doubling (acc == addend; the only other block with hundreds of multiply-adds besides the two of the
    # main path, which are the first two in program order) and the blocks outlined behind the loop
    heavy = [b_ for b_ in body if b_["v_mad_u64_u32"] >= 200]
    rare = [b_["label"] for b_ in heavy[2:]] + [b_["label"] for b_ in blocks[hi + 1:end + 1]]
    common = [b_ for b_ in body if b_["label"] not in rare]
    fmt = lambda bs: [{k: v for k, v in b_.items()} for b_ in bs if b_["instructions"]]
    return {"loop_head": blocks[lo]["label"],
            "loop_instructions_every_block": count(body, "instructions"), "loop_v_mad_u64_u32_every_block": count(body, "v_mad_u64_u32"),
            "loop_common_path_instructions": count(common, "instructions"), "loop_common_path_v_mad_u64_u32": count(common, "v_mad_u64_u32"),
            "loop_common_path_memory_instructions": count(common, "memory_instructions"),
            "mixed_addition_main_path_instructions": count(heavy[:2], "instructions"), "mixed_addition_main_path_v_mad_u64_u32": count(heavy[:2], "v_mad_u64_u32"),
            "rare_blocks_not_in_common_path": rare, "loop_blocks": fmt(body),
            "before_loop_instructions": count(head, "instructions"), "before_loop_v_mad_u64_u32": count(head, "v_mad_u64_u32"),
            "before_loop_memory_instructions": count(head, "memory_instructions"), "before_loop_blocks_of_20_or_more": fmt([b_ for b_ in head if b_["instructions"] >= 20]),
            "after_loop_instructions": count(tail, "instructions"), "after_loop_v_mad_u64_u32": count(tail, "v_mad_u64_u32"),
            "after_loop_blocks_of_20_or_more": fmt([b_ for b_ in tail if b_["instructions"] >= 20]),
            "vgprs": int(re.search(r"; NumVgprs: (\d+)", kernel).group(1)), "scratch_bytes": int(re.search(r"; ScratchSize: (\d+)", kernel).group(1)),
            "lds_bytes": int(re.search(r"; LDSByteSize: (\d+)", kernel).group(1)), "occupancy_waves_per_simd": int(re.search(r"; Occupancy: (\d+)", kernel).group(1))}


def loops(text):
    out = {"how": "hipcc -O3 --offload-arch=gfx950 -S; the first outermost loop (backward branch) that holds >= 900 v_mad_u64_u32 is the per-entry loop, with the "
                  "blocks laid out behind it that jump back into it; blocks in program order; 'skipped when s_cbranch_execz': executed by the whole wave as soon as ONE "
                  "lane needs it; common path = every block but the doubling and the outlined ones (tools/isa_counts.py --loops)"}
    for name, pat in (("k_accum_l0<false,true>", r"^_Z10k_accum_l0ILb0ELb1E.*?; Occupancy: \d+"), ("k_accum_runs<true>", r"^_Z12k_accum_runsILb1EE.*?; Occupancy: \d+"),
                      ("k_accum_runs<false>", r"^_Z12k_accum_runsILb0EE.*?; Occupancy: \d+")):
        out[name] = loop_tally(re.search(pat, text, re.S | re.M).group(0))
    print(json.dumps(out, indent=1))
    if "--write" in sys.argv:
        with open(os.path.join(REPO, "profiles", "accum_loop_isa_ledger.json"), "w") as f:
            json.dump(out, f, indent=1)


def main():
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "bpmi.s")
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-DBPMI_ISA_PROBE", "-S", "--cuda-device-only",
                               "-Wno-unused-command-line-argument", "-o", asm, SRC], stderr=subprocess.DEVNULL)
        text = open(asm).read()
    if "--loops" in sys.argv:
        return loops(text)
    m = re.search(r"^_Z10k_accum_l0ILb0E.*?; Occupancy: \d+", text, re.S | re.M)
    kernel = m.group(0)
    probe = re.search(r"^_Z16k_isa_probe_madd.*?; Occupancy: \d+", text, re.S | re.M).group(0)
    # the whole probe kernel is the main path plus the loads / stores of its operands and their address arithmetic;
    # memory instructions, waits and the kernel prologue / epilogue are tallied separately
    counts, other = collections.Counter(), collections.Counter()
    for ln in probe.splitlines():
        mm = INSTR.match(ln)
        if not mm:
            continue
        op = mm.group(1)
        if op.startswith(("global_", "s_load", "s_waitcnt", "s_endpgm", "buffer_", "flat_", "scratch_")):
            other[op] += 1
        else:
            counts[op] += 1
    total = sum(counts.values())
    vgpr = re.search(r"; NumVgprs: (\d+)", kernel).group(1)
    occ = re.search(r"; Occupancy: (\d+)", kernel).group(1)
    whole = sum(1 for ln in kernel.splitlines() if INSTR.match(ln))
    out = {"k_accum_l0_madd_main_path": {
        "instructions_per_madd": total,
        "v_mad_u64_u32_per_madd": counts.get("v_mad_u64_u32", 0),
        "s_nop_per_madd": counts.get("s_nop", 0),
        "by_mnemonic": dict(counts.most_common()),
        "probe_kernel_memory_and_wait_instructions": dict(other),
        "kernel_vgprs": int(vgpr), "kernel_occupancy_waves_per_simd": int(occ), "kernel_instructions_total": whole,
        "how": "hipcc -O3 --offload-arch=gfx950 -DBPMI_ISA_PROBE -S; every non-memory instruction of k_isa_probe_madd = xyzz_madd_pr + xyzz_madd_finish, the code k_accum_l0 inlines per sorted entry; the loop's own per-entry work (64-byte load, 8x32 -> 9x29 limb conversion, sign select, run-boundary test) is not in this count (tools/isa_counts.py)",
        "round_1_for_comparison": {"instructions_per_madd": 1953, "v_mad_u64_u32_per_madd": 942, "note": "same span measured on the round-1 code (commit c7275e6)"}}}
    print(json.dumps(out, indent=1))
    if "--write" in sys.argv:
        with open(os.path.join(REPO, "profiles", "r04_isa_counts.json"), "w") as f:
            json.dump(out, f, indent=1)
        with open(os.path.join(REPO, "profiles", "r04_isa_k_isa_probe_madd.s"), "w") as f:
            f.write(probe + "\n")


if __name__ == "__main__":
    main()
