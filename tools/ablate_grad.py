"""What a launch of the gradient kernel is made of (development aid): timing ablations, through
accbpg_debug_grad_variant, interleaved rounds in one process, minimum and median over the rounds.

Codes 3 and 10..13 ablate the schedule the kernel had before its k loop was split into a rectangular and a diagonal phase;
4 is the two-phase loop with every k-step on the block schedule, 0 the same loop with the rectangular steps and the first
five diagonal ones dealt out (production), 5 the dealt-out placement production does not use, 6 only the rectangular steps
dealt out; 20..23 ablate 4 and 30..33 ablate 0 (MFMAs only / MFMAs
and loads / MFMAs and fragment reads / everything but the counted wait and the barrier).  Every ablation computes wrong
results.

An ablation says something about the loop it ablates only if it compiled like it: `--isa FILE.s` (the output of
`hipcc --offload-arch=gfx950 -O3 -std=c++17 -S --cuda-device-only csrc/dopt_kernels.hip`) adds each instantiation's
private-segment size to the result, and a variant with scratch that the loop it ablates does not have is marked
"not interpreted".  `--isa-only` writes that table without touching a GPU."""
import argparse
import ctypes as C
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# code -> (description, template code CV of colnorm_glds_kernel, code of the loop it ablates)
CODES = {0: ("production (two phases, dealt out)", 256, None),
         4: ("two phases, block schedule", 256 | 1024, None),
         5: ("two phases, dealt out, the other placement", 256 | 2048, None),
         6: ("two phases, only the rectangular k-step dealt out", 256 | 8192, None),
         3: ("runtime skip, restart per row block", 256 | 512, None),
         10: ("restart schedule, rectangular k-steps only", 256 | 512 | 1, 3),
         11: ("restart schedule, diagonal k-steps only", 256 | 512 | 2, 3),
         12: ("restart schedule, MFMA only", 256 | 512 | 4, 3),
         13: ("restart schedule, no drain or restart between row blocks", 256 | 512 | 8, 3),
         20: ("block schedule, MFMA only", 256 | 1024 | 4096 | 7, 4),
         21: ("block schedule, MFMA and loads", 256 | 1024 | 4096 | 6, 4),
         22: ("block schedule, MFMA and fragment reads", 256 | 1024 | 4096 | 3, 4),
         23: ("block schedule, all but the counted wait and the barrier", 256 | 1024 | 4096 | 2, 4),
         30: ("dealt out, MFMA only", 256 | 4096 | 7, 0),
         31: ("dealt out, MFMA and loads", 256 | 4096 | 6, 0),
         32: ("dealt out, MFMA and fragment reads", 256 | 4096 | 3, 0),
         33: ("dealt out, all but the counted wait and the barrier", 256 | 4096 | 2, 0)}


def scratch_table(isa_path):
    """private-segment bytes of colnorm_glds_kernel<TileBig<true, false>, CV> per code, from the compiler's assembly"""
    lines = open(isa_path).read().split("\n")
    by_cv = {}
    for i, l in enumerate(lines):
        m = re.match(r"^(_ZN6accbpg\w*colnorm_glds_kernelINS_4TileILi256ELi128ELi64ELi128ELb1ELb0EEELi(\d+)EEE\w*):", l)
        if not m:
            continue
        for k in range(i, len(lines)):
            if ".amdhsa_private_segment_fixed_size" in lines[k]:
                by_cv[int(m.group(2))] = int(lines[k].split()[-1])
                break
    out = {}
    for code, (name, cv, of) in CODES.items():
        out[name] = {"code": code, "scratch_bytes": by_cv.get(cv)}
    for code, (name, cv, of) in CODES.items():
        if of is not None:
            base = by_cv.get(CODES[of][1])
            out[name]["ablates"] = CODES[of][0]
            out[name]["interpreted"] = base is not None and by_cv.get(cv) is not None and by_cv[cv] <= base
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=None)
    ap.add_argument("--isa", default=None, help="assembly of csrc/dopt_kernels.hip, or a JSON table written by --isa-only")
    ap.add_argument("--isa-only", action="store_true")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    table = None
    if args.isa:
        table = json.load(open(args.isa)) if args.isa.endswith(".json") else scratch_table(args.isa)
    if args.isa_only:
        txt = json.dumps(table, indent=1)
        print(txt)
        if args.out:
            open(args.out, "w").write(txt)
        return
    import numpy as np
    import torch
    import accbpg_and_fw_amd as acc
    from accbpg_and_fw_amd import _lib
    from accbpg_and_fw_amd.functions import _ptr
    lib = _lib.load()
    gen = torch.Generator(device="cuda").manual_seed(3)
    V = torch.randn(2048, 32768, dtype=torch.float64, device="cuda", generator=gen)
    x = torch.rand(32768, dtype=torch.float64, device="cuda", generator=gen) + 0.05
    x /= x.sum()
    f = acc.DOptimalObj(V)
    f.func_grad(x, 2)                                            # leaves the inverse factor the launches read
    g = torch.empty(32768, dtype=torch.float64, device="cuda")
    ms = C.c_double(0.0)
    out = {c: [] for c in CODES}
    for rnd in range(args.rounds):
        for c in CODES:
            _lib.check(lib.accbpg_debug_grad_variant(f._h, _ptr(g), c, args.iters, C.byref(ms)), "variant %d" % c)
            out[c].append(ms.value)
        print(rnd, {c: round(v[-1], 4) for c, v in out.items()}, flush=True)
    res = {"shape": [2048, 32768], "rounds": args.rounds, "launches_per_round": args.iters,
           "min_ms": {CODES[c][0]: min(v) for c, v in out.items()},
           "median_ms": {CODES[c][0]: float(np.median(v)) for c, v in out.items()},
           "rounds_ms": {CODES[c][0]: v for c, v in out.items()}}
    if table is not None:
        res["compiled"] = table
    print(json.dumps(res, indent=1))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
