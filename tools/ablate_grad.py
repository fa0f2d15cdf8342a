"""What a launch of the gradient kernel is made of (development aid): timing ablations, through
accbpg_debug_grad_variant, of the schedule the kernel had before its k loop was split into a rectangular and a diagonal
phase (wrong results except the first two), interleaved rounds, minimum over the rounds."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CODES = {0: "production (two phases, one pipeline per workgroup)", 3: "runtime skip, restart per row block",
         10: "restart schedule, rectangular k-steps only", 11: "restart schedule, diagonal k-steps only",
         12: "restart schedule, MFMA only", 13: "restart schedule, no drain or restart between row blocks"}


def main():
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
    for rnd in range(3):
        for c in CODES:
            _lib.check(lib.accbpg_debug_grad_variant(f._h, _ptr(g), c, 20, C.byref(ms)), "variant %d" % c)
            out[c].append(ms.value)
    res = {"shape": [2048, 32768], "min_ms": {CODES[c]: min(v) for c, v in out.items()},
           "rounds_ms": {CODES[c]: v for c, v in out.items()}}
    print(json.dumps(res, indent=1))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
