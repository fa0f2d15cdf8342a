"""The launch plans of a D-optimal handle are pure host logic (accbpg_and_fw_amd/csrc/dopt_plan.hpp): the Gram tile
list and its stream-K partition, the contributor lists of the fix-up, the inverse-merge plan, the job list of the
one-launch Cholesky.  The header is compiled alone with the host compiler, with a small main that plans the shapes of
tests/plan_cases.py and prints the plans.  They must (i) equal, array for array, what build_plans gave in the commit
before the header existed (tests/golden/dopt_plans_parent.npz, written from that commit by tools/gen_plan_golden.py), and
(ii) satisfy what any correct plan satisfies: every (tile, k-step) covered once, the fix-up's lists in k order and equal
to what the device walk leaves in slabs, every lower tile present once, every block of the inverse written once.
No GPU, nothing loaded into Python."""
import os
import shutil
import subprocess
import sys
from collections import Counter

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_DIR = os.path.join(ROOT, "accbpg_and_fw_amd", "csrc")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plan_cases as P  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "dopt_plans_parent.npz")

# the walk of every workgroup, cut with the header's own segment rule: one row (w, slot, entry, half, kb, ke, whole) per
# segment, in the order the device meets them
MAIN = r"""
#include "dopt_plan.hpp"
using namespace accbpg;
""" + P.DUMP_CPP + r"""
int main(int argc, char** argv) {
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    Case c;
    while (read_case(f, &c)) {
        printf("case %s\n", c.name);
        if (!strcmp(c.kind, "gram")) {
            GramPlanIn in;
            in.m = c.m; in.n = c.n; in.ldv = c.ldv; in.big = c.big; in.vec_ok = c.vec_ok; in.use_glds = c.use_glds;
            in.num_cu = c.num_cu; in.grid_cap = c.grid_cap; in.flags = c.flags;
            const GramPlan p = plan_gram(in);
            if (!p.ok) return 1;
            dump_scalar("chunks", p.chunks); dump_scalar("nc", p.nc); dump_scalar("want_block_copy", p.want_block_copy);
            dump_scalar("kiters", p.kiters); dump_scalar("has_duals", p.has_duals); dump_scalar("ntiles", (long long)p.tiles.size());
            dump_scalar("grid", p.grid); dump_scalar("per", p.per); dump_scalar("nslot", p.nslot);
            dump_scalar("tiny_k", p.tiny_k); dump_scalar("aligned", p.aligned); dump_scalar("whole_tiles", p.whole_tiles);
            dump_scalar("xcd_D", p.xcd_D); dump_scalar("rmax", GRAM_RMAX);
            dump_scalar("BM", c.big ? TILE_BIG_M : TILE_SMALL_M); dump_scalar("BN", c.big ? TILE_BIG_N : TILE_SMALL_N);
            dump_array("tiles", &p.tiles[0].rb, p.tiles.size() * 4);
            dump_array("ranges", p.ranges.data(), p.ranges.size());
            dump_array("cstart", p.cstart.data(), p.cstart.size());
            dump_array("contrib", p.contrib.data(), p.contrib.size());
            std::vector<long long> segs;
            for (int w = 0; w < p.grid; ++w) {
                int slot = 0;
                for (int r = 0; r < GRAM_RMAX; ++r) {
                    long long it = p.ranges[((size_t)w * GRAM_RMAX + r) * 2];
                    const long long it1 = p.ranges[((size_t)w * GRAM_RMAX + r) * 2 + 1];
                    while (it < it1) {
                        const long long e = it / p.kiters, off = it - e * p.kiters;
                        const GramSegK s = gram_segment_k(p.kiters, off, it1 - it, p.tiles[(size_t)e].d1 >= 0);
                        for (long long v : {(long long)w, (long long)slot, e, (long long)s.second, (long long)s.kb, (long long)s.ke, (long long)s.whole})
                            segs.push_back(v);
                        it += s.ke - s.kb;
                        ++slot;
                    }
                }
            }
            dump_array("segs", segs.data(), segs.size());
        } else {
            const double* L = (const double*)((uintptr_t)2 << 40);
            double *W = (double*)((uintptr_t)3 << 40), *T = (double*)((uintptr_t)4 << 40), *Pb = (double*)((uintptr_t)5 << 40);
            const MergePlan mp = plan_merges(c.m, L, W, T, Pb);
            const int nblk = (int)((c.m + NB - 1) / NB);
            const std::vector<CholJob> jobs = nblk <= CT_TMAX ? chol_jobs(nblk) : std::vector<CholJob>();
            const Bases bs = {{L, W, T, Pb}, c.m * c.m};
            dump_merges(bs, mp.ops.data(), mp.ops.size(), mp.reds.data(), mp.reds.size(), mp.stages.data(), mp.stages.size(),
                        jobs.data(), jobs.size());
            dump_scalar("NB", NB); dump_scalar("KP", KP); dump_scalar("KSPLIT_MIN", KSPLIT_MIN);
        }
    }
    return 0;
}
"""


def _compiler():
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        if name and shutil.which(name):
            return shutil.which(name)
    rocm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "clang++")
    assert os.path.exists(rocm), "no host C++ compiler found"
    return rocm


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    d = tmp_path_factory.mktemp("plan")
    (d / "main.cpp").write_text(MAIN)
    (d / "cases.txt").write_text(P.cases_text())
    exe = d / "plans"
    subprocess.check_call([_compiler(), "-std=c++17", "-O1", "-Wall", "-Werror", "-I", HEADER_DIR, str(d / "main.cpp"), "-o", str(exe)])
    P.GRAM_ARRAYS["segs"] = np.int64
    try:
        return P.parse(subprocess.check_output([str(exe), str(d / "cases.txt")], text=True))
    finally:
        del P.GRAM_ARRAYS["segs"]


def test_header_stands_alone():
    """No HIP include: the fixture compiled the header with the host compiler alone."""
    includes = [ln.strip() for ln in open(os.path.join(HEADER_DIR, "dopt_plan.hpp")) if ln.startswith("#include")]
    assert includes == ["#include <stdint.h>", "#include <algorithm>", "#include <vector>"]


def test_plans_equal_the_parents(plans):
    golden = np.load(GOLDEN)
    mine = P.pack(plans)
    assert set(golden.files) - {"rev"} == set(mine)
    assert os.path.getsize(GOLDEN) < 256 * 1024
    for k in sorted(mine):
        assert np.array_equal(golden[k], mine[k]), k
        assert golden[k].dtype == np.asarray(mine[k]).dtype, k


@pytest.mark.parametrize("case", P.GRAM_CASES, ids=[c["name"] for c in P.GRAM_CASES])
def test_shape_table_covers_its_branch(plans, case):
    """The table cannot quietly stop covering a branch of the planner."""
    p = plans[case["name"]]
    tile = "big" if case["big"] else "small"
    interior = case["vec_ok"] and case["m"] % p["BM"] == 0 and case["n"] % 16 == 0
    seen = dict(tile=tile, edge=int(not interior), duals=p["has_duals"], tiny_k=p["tiny_k"], xcd_D=p["xcd_D"],
                part="aligned" if p["aligned"] else "whole" if p["whole_tiles"] else "plain",
                **{k: p[k] for k in ("chunks", "want_block_copy", "ntiles", "nslot", "per")})
    assert {k: seen[k] for k in case["branch"]} == case["branch"]
    if seen["part"] != "plain" or tile == "small":
        assert p["xcd_D"] == 0


@pytest.mark.parametrize("case", P.GRAM_CASES, ids=[c["name"] for c in P.GRAM_CASES])
def test_gram_plan_invariants(plans, case):
    p = plans[case["name"]]
    kit, ntiles, grid, rmax = p["kiters"], p["ntiles"], p["grid"], p["rmax"]
    tiles = p["tiles"].reshape(ntiles, 4)
    dual = tiles[:, 2] >= 0
    # every (entry, unit) lies in exactly one range; a workgroup owns at most GRAM_RMAX of them
    assert p["ranges"].size == grid * rmax * 2
    r = p["ranges"].reshape(-1, 2)
    r = r[r[:, 1] > r[:, 0]]
    r = r[np.argsort(r[:, 0])]
    assert r[0, 0] == 0 and r[-1, 1] == ntiles * kit and np.array_equal(r[1:, 0], r[:-1, 1])
    # the walk: a workgroup's segments take the slab slots 0, 1, ... and there are at most nslot of them
    segs = p["segs"].reshape(-1, 7)
    per_wg = Counter(segs[:, 0].tolist())
    assert max(per_wg.values()) <= p["nslot"]
    for w, slot in segs[:, :2]:
        assert slot < per_wg[w]
    assert np.all(segs[:, 5] > segs[:, 4])
    assert not np.any(segs[:, 3][~dual[segs[:, 2]]])                # the second half exists for dual entries only
    seg_of = {(int(s[0]), int(s[1])): s for s in segs}
    assert len(seg_of) == len(segs)
    # what the device leaves in a slab: every segment of a dual entry, every partial one, and all of them when chunked
    in_slab = {k for k, s in seg_of.items() if dual[s[2]] or not s[6] or p["chunks"] > 1}
    cstart, contrib = p["cstart"], p["contrib"]
    assert cstart.size == 2 * ntiles + 1 and cstart[0] == 0 and np.all(np.diff(cstart) >= 0)
    listed = set()
    for e in range(ntiles):
        for half in range(2):
            lo, hi = cstart[2 * e + half], cstart[2 * e + half + 1]
            mine = [seg_of[(int(contrib[2 * i]), int(contrib[2 * i + 1]))] for i in range(lo, hi)]
            assert all(s[2] == e and s[3] == half for s in mine)
            assert [s[4] for s in mine] == sorted(s[4] for s in mine)           # added up in k order
            listed |= {(int(s[0]), int(s[1])) for s in mine}
            if half == 1 and not dual[e]:
                assert not mine
                continue
            # with the segments written straight to G they tile the k-steps of the tile (of the block) exactly
            direct = [s for s in segs[(segs[:, 2] == e) & (segs[:, 3] == half)] if (int(s[0]), int(s[1])) not in in_slab]
            cover = sorted((int(s[4]), int(s[5])) for s in mine + direct)
            end = kit // 2 if dual[e] else kit
            assert cover[0][0] == 0 and cover[-1][1] == end
            assert all(a[1] == b[0] for a, b in zip(cover, cover[1:]))
    assert listed == in_slab                                        # the lists match what the device walk writes
    assert cstart[-1] == len(in_slab)
    if p["chunks"] > 1:
        assert len(in_slab) == len(segs)
    # every lower tile of the m x m grid appears once; a dual entry stands for both of its odd diagonal blocks
    BM, BN = p["BM"], p["BN"]
    nrb, ncb = -(-case["m"] // BM), -(-case["m"] // BN)
    want = Counter((rb, cb) for rb in range(nrb) for cb in range(ncb) if cb * BN <= rb * BM + BM - 1)
    have = Counter()
    for rb, cb, d1, d2 in tiles.tolist():
        if d1 < 0:
            have[(rb, cb)] += 1
        else:
            assert d1 % 2 == 1 and d2 % 2 == 1 and BM == 2 * BN and kit % 2 == 0
            have[(d1 // 2, d1)] += 1
            have[(d2 // 2, d2)] += 1
    assert have == want
    assert p["has_duals"] == int(dual.any())


@pytest.mark.parametrize("m", P.MERGE_M)
def test_merge_plan_invariants(plans, m):
    p = plans["m%d" % m]
    NB, KP, KSPLIT_MIN = p["NB"], p["KP"], p["KSPLIT_MIN"]
    ops = [dict(zip(P.OP_FIELDS, row)) for row in p["ops"].reshape(-1, len(P.OP_FIELDS)).tolist()]
    reds = [dict(zip(P.RED_FIELDS, row)) for row in p["reds"].reshape(-1, len(P.RED_FIELDS)).tolist()]
    stages = p["stages"].reshape(-1, 5).tolist()
    T = -(-m // NB)
    # the stages are contiguous: products and reductions each run through their table in order
    nxt = [0, 0]
    for kind, begin, end, maxm, maxn in stages:
        assert begin == nxt[kind] and end > begin
        nxt[kind] = end
    assert nxt == [len(ops), len(reds)]
    Lb, Wb, Tb, Pb = (P.BASES[k] for k in "LWTP")
    written = Counter()                                             # blocks of W and T: (buffer, offset, rows, columns)
    split_lists = 0
    for i, (kind, begin, end, maxm, maxn) in enumerate(stages):
        if kind == 1:
            continue
        mine = ops[begin:end]
        assert maxm == max(o["M"] for o in mine) and maxn == max(o["N"] for o in mine)
        to_p = [o for o in mine if o["C_base"] == Pb]
        if not to_p:
            for o in mine:
                assert o["K"] == (o["N"] if o["tri"] == 1 else o["M"]) and o["koff"] == 0 and o["ldc"] == m
                written[(o["C_base"], o["C_off"], o["M"], o["N"])] += 1
            continue
        # a split list: all its products are, and the reduction stage behind it sums their pieces
        split_lists += 1
        assert len(to_p) == len(mine) and stages[i + 1][0] == 1
        rs = reds[stages[i + 1][1]:stages[i + 1][2]]
        pieces = sorted((o["C_off"], o["C_off"] + o["M"] * o["N"]) for o in mine)
        assert pieces[0][0] >= 0 and pieces[-1][1] <= m * m                     # Pbuf pieces end within m*m ...
        assert all(a[1] <= b[0] for a, b in zip(pieces, pieces[1:]))            # ... and are disjoint
        for r in rs:
            mine_r = [o for o in mine if r["P_off"] <= o["C_off"] < r["P_off"] + r["ns"] * r["M"] * r["N"]]
            assert r["P_base"] == Pb and len(mine_r) == r["ns"]
            for k, o in enumerate(sorted(mine_r, key=lambda o: o["C_off"])):
                assert (o["M"], o["N"], o["ldc"]) == (r["M"], r["N"], r["N"])
                assert o["K"] == KP and o["koff"] == k * KP and o["C_off"] == r["P_off"] + k * r["M"] * r["N"]
            total_k = sum(o["K"] for o in mine_r)                               # the K-pieces sum to the product's K
            assert total_k == (r["N"] if mine_r[0]["tri"] == 1 else r["M"]) and total_k >= KSPLIT_MIN
            written[(r["C_base"], r["C_off"], r["M"], r["N"])] += 1
        assert sum(r["ns"] for r in rs) == len(mine)
    # each W21 block of the binary tree (and the T1 beside it) is written by exactly one product or reduction
    want = Counter()
    span = 1
    while span < T:
        for g in range(0, T - span, 2 * span):
            r1, s1 = g * NB, span * NB
            r2 = r1 + s1
            s2 = min(span * NB, m - r2)
            want[(Wb, r2 * m + r1, s2, s1)] += 1
            want[(Tb, r2 * m + r1, s2, s1)] += 1
        span *= 2
    assert written == want
    # lists that are split: K >= KSPLIT_MIN in whole pieces.  64: no merges; 200 and 512: K stays below KSPLIT_MIN; 1024
    # and 2048: both lists of the levels of 8 (and 16) blocks; 1100: those of the level of 8 and the first of the top
    # level, whose second list has the ragged last block (K = 76) and is refused
    assert split_lists == {64: 0, 200: 0, 512: 0, 1100: 3, 1024: 2, 2048: 4}[m]
    if m == 64:
        assert not ops and not stages
