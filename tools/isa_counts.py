#!/usr/bin/env python3
"""Static counts of a kernel's gfx950 assembly (no GPU needed).

  hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S \
      -o wave.s antidote_ccrdt_amd/csrc/trmv_wave.hip
  tools/isa_counts.py wave.s [substring of the kernel symbol ...]

Per kernel: instructions by unit, scalar loads by width, for every scalar load
the distance (in instructions) to the first s_waitcnt that covers it
(lgkmcnt(0)), how many of those waits also had LDS operations in flight,
global instructions that take a 64-bit per-lane address (`off` in place of a
scalar base) against those with a scalar base, lane moves (v_readlane /
v_writelane: SGPR spills live there), and the resource lines of the metadata.
The per-key body is not separated from the chunk set-up: compare two builds,
not one build against the source.
"""
import re
import statistics
import sys


def kernels(path):
    name, body, out = None, [], {}
    for line in open(path):
        s = line.strip()
        m = re.match(r"^(_Z\w+):", line)
        if m and name is None:
            name, body = m.group(1), []
            continue
        if name is not None:
            if s.startswith(".amdhsa_kernel") or s.startswith(".section") and ".rodata" in s:
                out[name] = body
                name = None
                continue
            if not s or s.startswith((".", ";", "//")) or s.endswith(":"):
                continue
            body.append(s.split(";")[0].strip())
    return out


def meta(path):
    out, cur = {}, None
    keys = ("sgpr_count", "sgpr_spill_count", "vgpr_count", "vgpr_spill_count", "private_segment_fixed_size")
    for line in open(path):
        s = line.strip().lstrip("- ")
        if s.startswith(".name:"):
            cur = s.split()[-1]
        for k in keys:
            if s.startswith("." + k + ":"):
                out.setdefault(cur, {})[k] = int(s.split()[-1])
    return out


def count(body):
    c = dict(total=len(body), valu=0, salu=0, lds=0, glob=0, smem=0, waitcnt=0, lgkm0=0, lane_moves=0,
             glob_vaddr64=0, glob_saddr=0, lshl_add_u64=0, mad_u64_u32=0)
    widths, dist, pend, lds_pend, waits_smem, waits_smem_lds = {}, [], [], 0, 0, 0
    for i, ins in enumerate(body):
        op = ins.split()[0]
        if op.startswith("s_load_") or op.startswith("s_buffer_load_"):
            c["smem"] += 1
            widths[op] = widths.get(op, 0) + 1
            pend.append(i)
        elif op == "s_waitcnt":
            c["waitcnt"] += 1
            if "lgkmcnt(0)" in ins:
                c["lgkm0"] += 1
                if pend:
                    waits_smem += 1
                    waits_smem_lds += 1 if lds_pend else 0
                    dist += [i - p for p in pend]
                pend, lds_pend = [], 0
        elif op.startswith("ds_"):
            c["lds"] += 1
            lds_pend += 1
        elif op.startswith("global_") or op.startswith("flat_") or op.startswith("scratch_"):
            c["glob"] += 1
            if op.startswith("global_"):
                c["glob_vaddr64" if re.search(r"\boff\b", ins) else "glob_saddr"] += 1
        elif op.startswith("v_"):
            c["valu"] += 1
            if op in ("v_readlane_b32", "v_writelane_b32"):
                c["lane_moves"] += 1
            if op == "v_lshl_add_u64":
                c["lshl_add_u64"] += 1
            if op == "v_mad_u64_u32":
                c["mad_u64_u32"] += 1
        elif op.startswith("s_"):
            c["salu"] += 1
    c["smem_widths"] = widths
    c["waits_covering_smem"] = waits_smem
    c["of_those_with_lds_in_flight"] = waits_smem_lds
    if dist:
        c["smem_to_wait_median"] = statistics.median(dist)
        c["smem_to_wait_le1"] = sum(d <= 1 for d in dist)
        c["smem_to_wait_le3"] = sum(d <= 3 for d in dist)
    return c


def main():
    path, want = sys.argv[1], sys.argv[2:]
    md = meta(path)
    for name, body in kernels(path).items():
        if want and not any(w in name for w in want):
            continue
        print(name)
        for k, v in count(body).items():
            print(f"  {k:30s} {v}")
        for k, v in md.get(name, {}).items():
            print(f"  {k:30s} {v}")


if __name__ == "__main__":
    main()
