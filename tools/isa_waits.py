#!/usr/bin/env python3
"""Where a kernel waits for memory:  tools/isa_waits.py FILE.s KERNEL

FILE.s is a gfx950 listing (hipcc ... --cuda-device-only -S), KERNEL a substring of the mangled name that selects ONE kernel
(`k_ba_lin_fusedILb1` is k_ba_lin_fused<true>).  The listing is walked in program order, every conditional branch taken as not taken
(the straight line is the path of a lane that does all the work).  vmcnt is modelled as the hardware counts it on gfx9: every vector-memory
instruction (flat_/global_/buffer_/scratch_ load, store, atomic, LDS-DMA) enters one in-order queue, and `s_waitcnt vmcnt(N)` returns once at
most N entries are left.  For every s_waitcnt that names vmcnt the tool prints how many LOADS were outstanding in front of it and how many of
them it retires, in three stretches of a linearisation kernel:

  front    entry -> first tap load
  gather   first -> last tap load (the waits behind the last batch belong to it: up to the first store or barrier behind the last tap)
  back     behind the gather -> first s_barrier

A tap load is a 12-byte vector load (`*_load_dwordx3`) behind the wave's first LDS write and in front of its first 16-byte store: the taps'
coordinates travel through LDS before any tap is requested, and the Jacobian groups and records are written behind the last; the other 12-byte
loads of such a kernel (its chunk descriptor, pieces of a table) lie outside.  A kernel without such loads is reported as one stretch.

Also printed: flat_ instructions, scratch_ instructions, the longest run of tap loads without a vmcnt wait in between per batch, and the
register / scratch figures of the compiler's own report.  analyse() returns all of it as a dict (tests/test_lin_isa_cpu.py).
"""
import re
import sys

VM_RE = re.compile(r"^(flat|global|buffer|scratch)_(load|store|atomic)|^(tbuffer)_(load|store)")
WAIT_RE = re.compile(r"vmcnt\((\d+)\)")


def kernel_body(text, kernel):
    """(mangled name, instruction lines, trailer comment lines) of the one kernel whose name contains `kernel`"""
    lines = text.splitlines()
    starts = [(n, m.group(1)) for n, l in enumerate(lines) for m in [re.match(r"^(_Z\w+):", l)] if m and kernel in m.group(1)]
    names = sorted({nm for _, nm in starts})
    if len(names) != 1:
        raise SystemExit("isa_waits: %r selects %d kernels: %s" % (kernel, len(names), ", ".join(names)))
    n0 = starts[0][0]
    body, trailer = [], []
    n = n0 + 1
    while n < len(lines) and not lines[n].startswith(".Lfunc_end"):
        body.append(lines[n])
        n += 1
    while n < len(lines) and not re.match(r"^_Z\w+:", lines[n]) and len(trailer) < 60:
        trailer.append(lines[n])
        n += 1
    return names[0], body, trailer


def analyse(text, kernel):
    name, body, trailer = kernel_body(text, kernel)
    ins = []
    for l in body:
        s = l.split(";")[0].strip()
        if not s or s.endswith(":") or s.startswith("."):
            continue
        ins.append(s)
    # tap loads: dwordx3 loads behind the first LDS write, in front of the first 16-byte store
    first_ds_write = next((k for k, s in enumerate(ins) if s.startswith("ds_write")), None)
    first_st16 = next((k for k, s in enumerate(ins) if re.match(r"^(flat|global|buffer)_store_dwordx4\b", s)), len(ins))
    taps = [k for k, s in enumerate(ins)
            if first_ds_write is not None and first_ds_write < k < first_st16 and re.match(r"^(flat|global|buffer)_load_dwordx3\b", s)]
    first_tap = taps[0] if taps else None
    last_tap = taps[-1] if taps else None
    gather_end = None
    if taps:
        gather_end = next((k for k in range(last_tap + 1, len(ins)) if re.match(r"^(flat|global|buffer)_store|^s_barrier", ins[k])), len(ins))
    first_barrier = next((k for k, s in enumerate(ins) if s.startswith("s_barrier") and (gather_end is None or k >= gather_end)), len(ins))

    def stretch(k):
        if first_tap is None:
            return "all"
        if k < first_tap:
            return "front"
        if k < gather_end:
            return "gather"
        if k <= first_barrier:
            return "back"
        return "rest"

    queue = []   # outstanding vector-memory instructions, oldest first: True for a load
    waits = []   # dicts: index, stretch, n, loads outstanding, loads retired, text
    for k, s in enumerate(ins):
        m = VM_RE.match(s)
        if m:
            queue.append("load" in s.split()[0])
            continue
        if s.startswith("s_waitcnt"):
            w = WAIT_RE.search(s)
            if not w:
                continue
            n = int(w.group(1))
            out = sum(queue)
            keep = queue[max(0, len(queue) - n):] if n else []
            waits.append({"index": k, "stretch": stretch(k), "vmcnt": n, "loads_outstanding": out, "loads_retired": out - sum(keep), "text": s})
            queue = keep
    # batches of tap loads: maximal runs of taps with no vmcnt wait in between
    batches, run = [], 0
    wait_idx = {w["index"] for w in waits}
    tapset = set(taps)
    for k in range(first_tap or 0, (last_tap + 1) if taps else 0):
        if k in wait_idx:
            if run:
                batches.append(run)
            run = 0
        elif k in tapset:
            run += 1
    if run:
        batches.append(run)
    res = {"kernel": name, "waits": waits, "tap_loads": len(taps), "tap_batches": batches,
           "flat": [s for s in ins if s.startswith("flat_")], "scratch": [s for s in ins if s.startswith("scratch_")]}
    for st in ("front", "gather", "back", "all"):
        res["waits_" + st] = sum(1 for w in waits if w["stretch"] == st and w["loads_outstanding"] > 0)
    for key, pat in (("vgprs", r"; NumVgprs: (\d+)"), ("sgprs", r"; NumSgprs: (\d+)"), ("scratch_bytes", r"; ScratchSize: (\d+)"),
                     ("lds_bytes", r"; LDSByteSize: (\d+)"), ("occupancy", r"; Occupancy: (\d+)")):
        m = re.search(pat, "\n".join(trailer))
        res[key] = int(m.group(1)) if m else None
    return res


def main():
    if len(sys.argv) != 3:
        raise SystemExit(__doc__)
    r = analyse(open(sys.argv[1]).read(), sys.argv[2])
    print(r["kernel"])
    print("  VGPRs %s  SGPRs %s  scratch %s B  LDS %s B  waves/SIMD %s" % (r["vgprs"], r["sgprs"], r["scratch_bytes"], r["lds_bytes"], r["occupancy"]))
    print("  flat_ instructions %d   scratch_ instructions %d   tap loads %d in batches %s" % (len(r["flat"]), len(r["scratch"]), r["tap_loads"], r["tap_batches"]))
    for st in ("front", "gather", "back", "rest", "all"):
        ws = [w for w in r["waits"] if w["stretch"] == st]
        if not ws:
            continue
        print("  %-6s %d s_waitcnt naming vmcnt, %d with loads outstanding" % (st, len(ws), sum(1 for w in ws if w["loads_outstanding"] > 0)))
        for w in ws:
            print("    #%-5d %-34s loads outstanding %2d, retired %2d" % (w["index"], w["text"], w["loads_outstanding"], w["loads_retired"]))


if __name__ == "__main__":
    main()
