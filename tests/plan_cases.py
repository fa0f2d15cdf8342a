"""The shape table of the launch-plan tests, and the text format in which a small C++ program hands plans to Python.

Shared by tests/test_plan_cpu.py (plans from csrc/dopt_plan.hpp) and tools/gen_plan_golden.py (plans from build_plans as
a commit had it), so that both dump the same cases in the same way.  Nothing here needs a GPU."""
import hashlib

import numpy as np


def gram_case(m, n, ldv=None, force_big=False, use_glds=True, num_cu=256, grid_cap=0, flags=0, **branch):
    """One handle as accbpg_dopt_create sees it (capi.hip decides vec_ok and big this way); `branch` names what the
    planner does with it."""
    ldv = n if ldv is None else ldv
    vec_ok = ldv % 2 == 0                       # (the base address of V is 16-byte aligned)
    big = m >= 768 or (force_big and vec_ok and m >= 256 and m % 256 == 0 and n % 128 == 0)
    name = "g%dx%d" % (m, n)
    for tag, on in (("_ld%d" % ldv, ldv != n), ("_big", force_big), ("_noglds", not use_glds),
                    ("_cap%d" % grid_cap, grid_cap), ("_f%d" % flags, flags)):
        if on:
            name += tag
    return dict(name=name, m=m, n=n, ldv=ldv, big=int(big), vec_ok=int(vec_ok), use_glds=int(use_glds), num_cu=num_cu,
                grid_cap=grid_cap, flags=flags, branch=branch)


# part: how the unit ranges are cut (plain / aligned / whole); the other keys are checked where they are given
GRAM_CASES = [
    gram_case(64, 64, tile="small", edge=0, part="plain"),
    gram_case(200, 333, tile="small", edge=1, part="plain"),
    gram_case(192, 640, tile="small", edge=0, part="plain"),
    gram_case(320, 48, tile="small", part="plain", per=1, tiny_k=0),    # three k-steps: a workgroup per (tile, k-step)
    gram_case(8192, 48, tile="big", part="whole", tiny_k=1, per=3),    # tiny K: more tiles than workgroups, one tile each
    gram_case(512, 1024, force_big=True, tile="big", duals=1, part="plain"),
    gram_case(1024, 4096, tile="big", duals=1, part="plain", xcd_D=9),
    gram_case(1280, 4096, tile="big", duals=1, part="plain", xcd_D=7),
    gram_case(1024, 4096, grid_cap=64, tile="big", part="aligned"),
    gram_case(1024, 4096, grid_cap=32, tile="big", part="aligned"),
    gram_case(2048, 4096, tile="big", part="aligned", nslot=3),
    gram_case(2560, 8192, tile="big", part="aligned", nslot=4),     # per/rem + 2 at the GRAM_RMAX bound
    gram_case(2048, 32768, use_glds=False, tile="big", part="aligned", duals=0, ntiles=72),
    gram_case(4096, 4096, tile="big", part="whole", ntiles=264),
    gram_case(8192, 2048, tile="big", part="whole", nslot=6),
    gram_case(8192, 2048, flags=1, tile="big", part="plain", ntiles=1040),
    gram_case(768, 65536, tile="big", chunks=2),
    gram_case(768, 65536, flags=4, tile="big", chunks=1),
    gram_case(8192, 65536, ldv=131072, tile="big", part="whole", chunks=2, want_block_copy=1),
]
MERGE_M = [64, 200, 512, 1024, 1100, 2048]
FULL_M = 2560                                   # arrays of larger shapes are kept as SHA-256

GRAM_ARRAYS = {"tiles": np.int32, "ranges": np.int64, "cstart": np.int32, "contrib": np.int32}
GRAM_SCALARS = ["chunks", "nc", "want_block_copy", "kiters", "has_duals", "ntiles", "grid", "per", "nslot"]
MERGE_ARRAYS = {"ops": np.int64, "reds": np.int64, "stages": np.int64, "jobs": np.int32}
OP_FIELDS = ["A_base", "A_off", "B_base", "B_off", "C_base", "C_off", "lda", "ldb", "ldc", "M", "N", "K", "lower_only",
             "tri", "koff", "alpha", "beta"]
RED_FIELDS = ["C_base", "C_off", "P_base", "P_off", "ldc", "M", "N", "ns"]
BASES = {"L": 0, "W": 1, "T": 2, "P": 3}


def cases_text():
    lines = []
    for c in GRAM_CASES:
        lines.append("gram %(name)s %(m)d %(n)d %(ldv)d %(big)d %(vec_ok)d %(use_glds)d %(num_cu)d %(grid_cap)d %(flags)d" % c)
    for m in MERGE_M:
        lines.append("merge m%d %d" % (m, m))
    return "\n".join(lines) + "\n"


# C++ shared by the two programs: reading the case file, and writing scalars, arrays and merge plans.  A pointer of a
# merge plan is written as (which buffer, offset in doubles).
DUMP_CPP = r"""
#include <stdio.h>
#include <string.h>
#include <vector>
struct Case { char kind[16], name[64]; long long m, n, ldv; int big, vec_ok, use_glds, num_cu, grid_cap, flags; };
static bool read_case(FILE* f, Case* c) {
    memset(c, 0, sizeof(*c));
    if (fscanf(f, "%15s %63s %lld", c->kind, c->name, &c->m) != 3) return false;
    if (!strcmp(c->kind, "merge")) { c->n = c->ldv = c->m; c->vec_ok = c->use_glds = 1; c->num_cu = 256; c->big = c->m >= 768; return true; }
    return fscanf(f, "%lld %lld %d %d %d %d %d %d", &c->n, &c->ldv, &c->big, &c->vec_ok, &c->use_glds, &c->num_cu,
                  &c->grid_cap, &c->flags) == 8;
}
static void dump_scalar(const char* key, long long v) { printf("scalar %s %lld\n", key, v); }
template <class T>
static void dump_array(const char* key, const T* p, size_t n) {
    printf("array %s %zu", key, n);
    for (size_t i = 0; i < n; ++i) printf(" %lld", (long long)p[i]);
    printf("\n");
}
struct Bases { const double* b[4]; long long mm; };     // L, W, T, P: m*m doubles each
static void put_ptr(std::vector<long long>& out, const Bases& bs, const double* p) {
    for (int i = 0; i < 4; ++i)
        if (p >= bs.b[i] && p - bs.b[i] < bs.mm) { out.push_back(i); out.push_back((long long)(p - bs.b[i])); return; }
    out.push_back(-1); out.push_back(0);
}
template <class Op, class Red, class Stage, class Job>
static void dump_merges(const Bases& bs, const Op* ops, size_t nops, const Red* reds, size_t nreds, const Stage* st,
                        size_t nst, const Job* jobs, size_t njobs) {
    std::vector<long long> o, r, s, j;
    for (size_t i = 0; i < nops; ++i) {
        put_ptr(o, bs, ops[i].A); put_ptr(o, bs, ops[i].B); put_ptr(o, bs, ops[i].C);
        for (long long v : {(long long)ops[i].lda, (long long)ops[i].ldb, (long long)ops[i].ldc, (long long)ops[i].M,
                            (long long)ops[i].N, (long long)ops[i].K, (long long)ops[i].lower_only, (long long)ops[i].tri,
                            (long long)ops[i].koff, (long long)ops[i].alpha, (long long)ops[i].beta})
            o.push_back(v);
    }
    for (size_t i = 0; i < nreds; ++i) {
        put_ptr(r, bs, reds[i].C); put_ptr(r, bs, reds[i].P);
        for (long long v : {(long long)reds[i].ldc, (long long)reds[i].M, (long long)reds[i].N, (long long)reds[i].ns}) r.push_back(v);
    }
    for (size_t i = 0; i < nst; ++i)
        for (long long v : {(long long)st[i].kind, (long long)st[i].begin, (long long)st[i].end, (long long)st[i].maxm, (long long)st[i].maxn})
            s.push_back(v);
    for (size_t i = 0; i < njobs; ++i) { j.push_back(jobs[i].i); j.push_back(jobs[i].j); }
    dump_array("ops", o.data(), o.size());
    dump_array("reds", r.data(), r.size());
    dump_array("stages", s.data(), s.size());
    dump_array("jobs", j.data(), j.size());
}
"""


def parse(text):
    """{case name: {key: int or 1-d array}} from a program's output"""
    out, cur = {}, None
    for line in text.splitlines():
        f = line.split()
        if f[0] == "case":
            cur = out.setdefault(f[1], {})
        elif f[0] == "scalar":
            cur[f[1]] = int(f[2])
        elif f[0] == "array":
            dtype = GRAM_ARRAYS.get(f[1]) or MERGE_ARRAYS[f[1]]
            assert len(f) == 3 + int(f[2]), (f[1], f[2], len(f))
            cur[f[1]] = np.array([int(v) for v in f[3:]], dtype=np.int64).astype(dtype)
        else:
            raise ValueError(line)
    return out


def digest(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)


def pack(plans):
    """The arrays of a stored-plan file: `<case>/<key>`, the arrays of the shapes above FULL_M as `<case>/<key>.sha256`"""
    rec = {}
    for c in GRAM_CASES:
        p = plans[c["name"]]
        for k in GRAM_SCALARS:
            rec["%s/%s" % (c["name"], k)] = np.int64(p[k])
        for k in GRAM_ARRAYS:
            if c["m"] <= FULL_M:
                rec["%s/%s" % (c["name"], k)] = p[k]
            else:
                rec["%s/%s.sha256" % (c["name"], k)] = digest(p[k])
                rec["%s/%s.len" % (c["name"], k)] = np.int64(p[k].size)
    for m in MERGE_M:
        for k in MERGE_ARRAYS:
            rec["m%d/%s" % (m, k)] = plans["m%d" % m][k]
    return rec


# ---- one evaluation per upload path of build_plans, compared bit for bit with the commit before the planner moved
# (tests/test_gpu_plan_parity.py, tools/gen_plan_parity_golden.py): small tiles with edges, the D-stride XCD order, the
# aligned ranges, whole tiles, two column blocks, and a batch (capped grid, the batch's op tables)
PARITY_CASES = [(200, 333, 1), (1024, 4096, 1), (2048, 4096, 1), (4096, 4096, 1), (768, 65536, 1), (1024, 4096, 4)]


def parity_name(case):
    return "%dx%d" % case[:2] + ("_batch%d" % case[2] if case[2] > 1 else "")


def parity_evaluate(acc, lib, case):
    """[(f, g)] of func_grad(x, 2) for the K instances of a case (K > 1: one DOptimalBatch call)"""
    import torch
    m, n, K = case
    rng = np.random.RandomState(1000 + m + n + K)
    Vs = [torch.from_numpy(rng.standard_normal((m, n))).cuda() for _ in range(K)]
    X = rng.rand(K, n) + 0.01
    X /= X.sum(axis=1, keepdims=True)
    X = torch.from_numpy(X).cuda()
    if K == 1:
        f = acc.DOptimalObj(Vs[0], _shard=(m >= n))         # (the square case: the form that takes m = n)
        lib.accbpg_dopt_value_reuse(f._h, 0)
        fv, g = f.func_grad(X[0], 2)
        return [(float(fv), g.cpu().numpy())]
    batch = acc.DOptimalBatch(Vs)
    fv, G = batch.func_grad(X, 2)
    G = G.cpu().numpy()
    return [(float(fv[i]), G[i]) for i in range(K)]


def parity_record(case, results):
    """What is kept of a case: f, the SHA-256 of g's bytes, g's first and last 16 entries (per instance)"""
    rec = {}
    for i, (fv, g) in enumerate(results):
        key = "%s/%d/" % (parity_name(case), i)
        g = np.ascontiguousarray(g, dtype=np.float64)
        rec[key + "f"] = np.float64(fv)
        rec[key + "g.sha256"] = digest(g)
        rec[key + "g.head"] = g[:16].copy()
        rec[key + "g.tail"] = g[-16:].copy()
    return rec
