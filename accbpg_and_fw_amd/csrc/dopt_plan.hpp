// Launch plans of a D-optimal handle: the Gram tile list and its stream-K partition, the contributor lists of the Gram
// fix-up, the inverse-merge plan, the job list of the one-launch Cholesky.  Pure integer logic in plain C++17: no HIP
// include, nothing allocated on a device.  dopt_kernels.hip plans with these functions and uploads what they return
// (build_plans); tests/test_plan_cpu.py compiles the header alone with the host compiler.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace accbpg {

constexpr int BK = 16;          // depth of a k-step (doubles) of the MFMA tile engine (mfma_tile.hpp)
constexpr int NB = 64;          // Cholesky / inverse block size
constexpr int TILE_BIG_M = 256, TILE_BIG_N = 128;       // workgroup tiles of the Gram / gradient products (mfma_tile.hpp)
constexpr int TILE_SMALL_M = 64, TILE_SMALL_N = 64;
constexpr int GRAM_RMAX = 4;    // unit ranges a workgroup can own (wg_ranges[w][r] = {first, end})
constexpr int64_t GRAM_NC = 32768;                      // columns of one column block of a long-row Gram matrix
constexpr int64_t KP = 256, KSPLIT_MIN = 512;           // inverse merges: K piece of a split product, smallest K that is split
constexpr int CT_TMAX = 32;     // block columns the one-launch Cholesky handles

// one product of the batched small-GEMM kernel: C = alpha * A * op(B) + beta * C
struct GemmOp {
    const double* A;
    const double* B;
    double* C;
    int64_t lda, ldb, ldc;
    int32_t M, N, K;
    int32_t lower_only;     // skip tiles / elements strictly above the diagonal of C
    int32_t tri;            // bit 0: B[k][col] is zero for k < col; bit 1: A[row][k] is zero for k > row (k ranges are cut)
    int32_t koff;           // k index of this op's first k-step in the coordinates of those triangles (split-K pieces)
    double alpha, beta;
};

// sum of split-K partial products: C[r][c] = sum_p P[p*M*N + r*N + c]
struct RedOp {
    double* C;
    const double* P;
    int64_t ldc;
    int32_t M, N, ns, pad;
};

// entry of the Gram tile list: one BM x BN tile (d1 < 0), or a pair of 128 x 128 diagonal blocks d1, d2
// (128-block indices) that run as "dual" tiles over half of K each (mfma_tile.hpp)
struct TileRC {
    int32_t rb, cb;
    int32_t d1 = -1, d2 = -1;
};

struct CholJob { int i, j; };                     // i == j: owner of the diagonal tile (and of (i, i-1))

// launch list of the inverse merges: kind 0 = products ops[begin, end), kind 1 = partial-sum reductions red[begin, end)
struct MergeStage { int kind, begin, end, maxm, maxn; };

// The k-steps of one stream-K segment.  A workgroup that still owns `len` units from offset `off` of an entry covers, of
// a BM x BN tile, the k-steps [off, min(kiters, off + len)); of a dual entry, whose two 128 x 128 blocks take kiters/2
// units each, the k-steps [kb, ke) of the first or the second block, counted from that block's first.  `whole`: the
// segment is all of its tile (or block), so a lone tile's accumulators go straight to G.  This is the host's copy of
// the rule by which the device walk cuts its ranges (gram_segment in dopt_kernels.hip): the replay of plan_gram and the
// invariants of tests/test_plan_cpu.py walk with it.
struct GramSegK {
    int64_t kb, ke;
    bool second, whole;
};
inline GramSegK gram_segment_k(int64_t kiters, int64_t off, int64_t len, bool dual) {
    GramSegK s;
    if (!dual) {
        s.second = false;
        s.kb = off;
        s.ke = kiters < off + len ? kiters : off + len;
        s.whole = (s.kb == 0 && s.ke == kiters);
    } else {
        const int64_t half = kiters >> 1;
        s.second = off >= half;
        s.kb = s.second ? off - half : off;
        s.ke = half < s.kb + len ? half : s.kb + len;
        s.whole = (s.kb == 0 && s.ke == half);
    }
    return s;
}

// development switches of the planner (accbpg_debug_plan_flags): bit 0 = plain stream-K ranges also where there are
// more tiles than workgroups (A/B of the whole-tile partition), bit 2 = long rows in one column block, bit 3 = no
// block-by-block copy of V
struct GramPlanIn {
    int64_t m = 0, n = 0, ldv = 0;
    bool big = false, vec_ok = false, use_glds = true;
    int num_cu = 256;
    int grid_cap = 0;           // stream-K workgroups of one instance of a batch (0: the whole chip)
    int flags = 0;
};
struct GramPlan {
    bool ok = true;
    int chunks = 1;             // column blocks of V the Gram matrix is formed over (one launch each)
    int64_t nc = 0;             // columns per block
    bool want_block_copy = false;   // the rows of V lie far enough apart for a copy stored block by block to pay
    int64_t kiters = 0;
    bool has_duals = false;
    std::vector<TileRC> tiles;
    int grid = 0, per = 0;
    std::vector<int64_t> ranges;    // [grid][GRAM_RMAX][2]
    int nslot = 1;
    std::vector<int32_t> cstart, contrib;   // per (entry, half): first pair of contrib; (workgroup, slab slot) pairs in k order
    // which partition was chosen (for tests and tools; the launches read none of these)
    bool tiny_k = false, aligned = false, whole_tiles = false;
    int xcd_D = 0;              // stride of the D-stride XCD order (0: the list was left as it was)
};

namespace plan_detail {

inline int64_t& range_lo(std::vector<int64_t>& ranges, int w, int r) { return ranges[((size_t)w * GRAM_RMAX + r) * 2]; }
inline int64_t& range_hi(std::vector<int64_t>& ranges, int w, int r) { return ranges[((size_t)w * GRAM_RMAX + r) * 2 + 1]; }

// 256x128 tiles: the tile (rb, 2rb+1) next to the diagonal holds one useful 128 x 128 block, the odd
// diagonal block 2rb+1, under 128 rows that lie strictly above the diagonal.  On the direct-to-LDS
// path those blocks run as dual tiles instead (half of K each at full MFMA work), two per entry.
inline std::vector<TileRC> tile_list(int nrb, int ncb, int BM, int BN, bool duals, bool* has_duals) {
    std::vector<TileRC> tl;
    std::vector<int> lone;
    for (int rb = 0; rb < nrb; ++rb)
        for (int cb = 0; cb < ncb; ++cb)
            if ((int64_t)cb * BN <= (int64_t)rb * BM + BM - 1) {
                if (duals && cb == 2 * rb + 1) lone.push_back(cb);
                else tl.push_back(TileRC{rb, cb});
            }
    for (size_t i = 0; i + 1 < lone.size(); i += 2)
        tl.push_back(TileRC{lone[i] / 2, lone[i], lone[i], lone[i + 1]});
    if (lone.size() & 1) tl.push_back(TileRC{lone.back() / 2, lone.back()});   // odd one out: ordinary tile
    *has_duals = lone.size() >= 2;
    return tl;
}

// compact order of the entries: 4 x 8 blocks of tiles
inline void sort_compact_4x8(std::vector<TileRC>& tl) {
    std::stable_sort(tl.begin(), tl.end(), [](const TileRC& a, const TileRC& b) {
        const int ka[4] = {a.rb / 4, a.cb / 8, a.rb, a.cb}, kb[4] = {b.rb / 4, b.cb / 8, b.rb, b.cb};
        for (int i = 0; i < 4; ++i)
            if (ka[i] != kb[i]) return ka[i] < kb[i];
        return false;
    });
}

// When a tile holds several
// whole ranges (q = kiters / per >= 1, remainder rem > 0) the ranges are instead ALIGNED to the
// tiles: every tile is cut at 0, per, .., q*per, so that all workgroups of "class" j start at k-step
// j*per of their tile and stream the same columns of V at the same time; the q*ntiles body pieces
// are dealt to the XCDs (workgroup id mod 8, round-robin placement -- speed only, never correctness)
// 32 at a time in an order in which 32 consecutive tiles form a compact block (few distinct row and
// column panels -> shared through that XCD's L2), and the remainders [q*per, kiters) are walked by
// the last workgroups as one contiguous stream.
inline bool ranges_aligned(std::vector<TileRC>& tl, std::vector<int64_t>& ranges, int grid, int64_t per, int64_t kit) {
    const int ntiles = (int)tl.size();
    const int64_t q = kit / per, rem = kit % per;
    sort_compact_4x8(tl);
    const int nbody = (int)(ntiles * q);
    const int px = (grid % 8 == 0) ? grid / 8 : 0;          // workgroups per XCD
    auto wg_of = [&](int i) { return px ? (i / px) + 8 * (i % px) : i; };
    int idx = 0;
    for (int64_t j = 0; j < q; ++j)
        for (int e = 0; e < ntiles; ++e, ++idx) {
            const int w = wg_of(idx);
            range_lo(ranges, w, 0) = (int64_t)e * kit + j * per;
            range_hi(ranges, w, 0) = (int64_t)e * kit + (j + 1) * per;
        }
    // remainders: tail-workgroup t covers the concatenated tails' units [t*per, (t+1)*per)
    const int64_t tail_total = (int64_t)ntiles * rem;
    for (int t = 0; nbody + t < grid; ++t) {
        const int w = wg_of(nbody + t);
        int64_t u = (int64_t)t * per;
        const int64_t u1 = std::min(u + per, tail_total);
        int r = 0;
        while (u < u1) {
            const int64_t e = u / rem, off = u - e * rem;
            const int64_t len = std::min(rem - off, u1 - u);
            if (r >= GRAM_RMAX) return false;               // cannot happen: per / rem + 2 <= GRAM_RMAX
            range_lo(ranges, w, r) = e * kit + q * per + off;
            range_hi(ranges, w, r) = e * kit + q * per + off + len;
            ++r;
            u += len;
        }
    }
    return true;
}

// More tiles than workgroups (m >= 4096 on 256 CUs; BASELINE config 5: 1056 entries): plain stream-K would hand
// every workgroup a contiguous range of 4.1 tiles that starts somewhere inside a tile, so no two workgroups ever
// stream the same columns of V at the same time and every k-step of every workgroup comes from HBM (measured at
// (8192,262144): 0.67 of the MFMA peak, against 0.84 at (8192,32768) where the Infinity Cache still covers the
// offsets).  Instead every workgroup gets `wt` WHOLE tiles, which it walks from k = 0 in step with all the others,
// and the workgroups of one XCD (id mod 8 under round-robin placement -- speed only, never correctness) hold, at
// every one of the wt phases, a compact 4 x 8 block of tiles: 4 row panels + 8 column panels feed 32 tiles through
// that XCD's L2.  The ntiles - wt*grid entries left over are cut into equal pieces, one per workgroup (the
// stream-K tail: a few percent of the work).
inline void ranges_whole_tiles(std::vector<TileRC>& tl, std::vector<int64_t>& ranges, int grid, int64_t kit) {
    const int ntiles = (int)tl.size();
    sort_compact_4x8(tl);
    const int wt = ntiles / grid, B = grid / 8;
    const int nbody = wt * grid;
    std::vector<TileRC> perm(tl);
    for (int pph = 0; pph < wt; ++pph)
        for (int xcd = 0; xcd < 8; ++xcd)
            for (int sl = 0; sl < B; ++sl) {
                const int w = 8 * sl + xcd;
                perm[(size_t)wt * w + pph] = tl[((size_t)pph * 8 + xcd) * B + sl];
            }
    tl.swap(perm);
    const int64_t tail_total = (int64_t)(ntiles - nbody) * kit;
    const int64_t tail_per = (tail_total + grid - 1) / grid;
    for (int w = 0; w < grid; ++w) {
        range_lo(ranges, w, 0) = (int64_t)wt * w * kit;
        range_hi(ranges, w, 0) = (int64_t)wt * (w + 1) * kit;
        const int64_t t0 = std::min((int64_t)w * tail_per, tail_total), t1 = std::min((int64_t)(w + 1) * tail_per, tail_total);
        range_lo(ranges, w, 1) = (int64_t)nbody * kit + t0;
        range_hi(ranges, w, 1) = (int64_t)nbody * kit + t1;
    }
}

// Plain stream-K hands workgroup w the contiguous range [w*per, (w+1)*per).
inline void ranges_plain(std::vector<int64_t>& ranges, int grid, int64_t per, int64_t total) {
    for (int w = 0; w < grid; ++w) {
        range_lo(ranges, w, 0) = std::min((int64_t)w * per, total);
        range_hi(ranges, w, 0) = std::min((int64_t)(w + 1) * per, total);
    }
}

// XCD-aware order.  Workgroups whose ranges start a whole number of tiles apart run the same
// k-step at the same time; with `per` steps per workgroup those are workgroups dw = kiters/g apart
// (g = gcd(per, kiters)), D = per/g tiles apart, and when dw is a multiple of 8 they share an XCD
// (round-robin placement: speed only, never correctness).  Arrange the list so that positions
// i, i+D, i+2D, ... hold a compact 2 x 4 block of tiles (2 A panels + 4 B panels feed 8 tiles),
// which those workgroups then stream through the same L2 together.
// Returns D, or 0 when the list stays as it is.
inline int xcd_stride_order(std::vector<TileRC>& tl, int nrb, int ncb, int64_t per, int64_t kit) {
    auto gcd64 = [](int64_t a, int64_t b) { while (b) { int64_t t = a % b; a = b; b = t; } return a; };
    const int64_t g = gcd64(per, kit);
    const int64_t D = per / g, dw = kit / g;
    const int nt = (int)tl.size();
    if (!(D > 1 && D < nt && nt % D == 0 && dw % 8 == 0)) return 0;
    const int gs = (int)(nt / D);
    // sequence in which consecutive runs are compact: row-block pairs, then 4 column blocks at a time
    std::vector<TileRC> seq;
    std::vector<char> used(tl.size(), 0);
    auto find = [&](int rb, int cb) {
        for (size_t i = 0; i < tl.size(); ++i)
            if (!used[i] && tl[i].rb == rb && tl[i].cb == cb) return (int)i;
        return -1;
    };
    const int bcols = (gs >= 2 && gs % 2 == 0) ? gs / 2 : 4;      // 2 x (gs/2) blocks fill one group
    for (int rp = nrb - 2 + (nrb & 1); rp >= -1; rp -= 2)
        for (int c4 = 0; c4 < ncb; c4 += bcols)
            for (int dr = 0; dr < 2; ++dr)
                for (int dc = 0; dc < bcols; ++dc) {
                    const int rb = rp + dr, cb = c4 + dc;
                    if (rb < 0 || rb >= nrb || cb >= ncb) continue;
                    // only full 2x4 blocks first; ragged remainders are appended below
                    const int i = find(rb, cb);
                    if (i >= 0 && find(rp + (1 - dr), cb) != -2) { used[i] = 1; seq.push_back(tl[i]); }
                }
    for (size_t i = 0; i < tl.size(); ++i)
        if (!used[i]) seq.push_back(tl[i]);
    std::vector<TileRC> perm(tl.size());
    for (int i = 0; i < (int)D; ++i)
        for (int j = 0; j < gs; ++j) perm[(size_t)D * j + i] = seq[(size_t)i * gs + j];
    tl.swap(perm);
    return (int)D;
}

// Replay every workgroup's walk (the device splits a range at tile and dual-half boundaries the same
// way): slab slot of each segment = its ordinal in the walk; contributors of each tile in k order.
// A segment that is a lone tile's whole K goes straight to G and is no contributor, unless the handle is chunked
// (every launch of a chunked handle leaves all its segments in slabs, which the fix-up adds to G).
inline void replay_contributors(GramPlan& p) {
    struct Contrib { int64_t kb; int w, slot; };
    std::vector<std::vector<Contrib>> cl(p.tiles.size() * 2);
    const int64_t kit = p.kiters;
    int nslot = 1;
    for (int w = 0; w < p.grid; ++w) {
        int seg = 0;
        for (int r = 0; r < GRAM_RMAX; ++r) {
            int64_t it = range_lo(p.ranges, w, r);
            const int64_t it1 = range_hi(p.ranges, w, r);
            while (it < it1) {
                const int64_t e = it / kit, off = it - e * kit;
                const bool dual = p.tiles[(size_t)e].d1 >= 0;
                const GramSegK s = gram_segment_k(kit, off, it1 - it, dual);
                if (dual || !s.whole || p.chunks > 1) cl[(size_t)e * 2 + (s.second ? 1 : 0)].push_back(Contrib{s.kb, w, seg});
                it += s.ke - s.kb;
                ++seg;
            }
        }
        nslot = std::max(nslot, seg);
    }
    p.nslot = nslot;
    p.cstart.assign(cl.size() + 1, 0);
    p.contrib.clear();
    for (size_t i = 0; i < cl.size(); ++i) {
        std::sort(cl[i].begin(), cl[i].end(), [](const Contrib& a, const Contrib& b) { return a.kb < b.kb; });
        for (const Contrib& c : cl[i]) { p.contrib.push_back(c.w); p.contrib.push_back(c.slot); }
        p.cstart[i + 1] = (int32_t)(p.contrib.size() / 2);
    }
    if (p.contrib.empty()) p.contrib.push_back(0);
}

}  // namespace plan_detail

// Gram tile list (lower tiles), stream-K partition and fix-up lists of one handle
inline GramPlan plan_gram(const GramPlanIn& in) {
    using namespace plan_detail;
    GramPlan p;
    const int64_t m = in.m;
    const bool interior256 = in.vec_ok && (m % 256 == 0) && (in.n % BK == 0);
    const int BM = in.big ? TILE_BIG_M : TILE_SMALL_M;
    const int BN = in.big ? TILE_BIG_N : TILE_SMALL_N;
    const int nrb = (int)((m + BM - 1) / BM), ncb = (int)((m + BN - 1) / BN);
    // Long rows: the Gram matrix is formed column block by column block of V (one launch each, added up in G).  Over a
    // pass of 16384 k-steps the workgroups of a launch drift apart and stop sharing their panels of V through L2: at
    // (8192,262144) one launch reached 0.68 of the MFMA peak, the (8192,32768) shape 0.86 -- so rows of 65536 columns or
    // more are cut into blocks of 32768 (which is also what the eight ranks of BASELINE config 5 hold each).
    p.chunks = 1;
    p.nc = in.n;
    if (!(in.flags & 4) && in.big && interior256 && in.use_glds && in.n >= 2 * GRAM_NC && in.n % GRAM_NC == 0) {
        p.chunks = (int)(in.n / GRAM_NC);
        p.nc = GRAM_NC;
        // Rows a megabyte or more apart: a tile of the Gram kernel streams 384 rows of V at once, and with that stride
        // every one of them sits in a page of its own -- measured on one (8192, 32768) column block: 32.5 ms with rows
        // 256 or 512 KiB apart, 34.6 ms at 1 MiB, 40.4 ms at 2 MiB (`tools/gram_stride.py`,
        // profiles/r03_gram_stride.json).  The handle then keeps a copy of V stored block by block ([block][row][32768
        // columns], made once, when the plans are built) and the Gram launches read that; everything else keeps reading
        // the caller's V, which must not change while the handle lives.
        p.want_block_copy = !(in.flags & 8) && in.ldv * (int64_t)sizeof(double) >= (1 << 20);
    }
    p.kiters = (p.nc + BK - 1) / BK;
    const int64_t kit = p.kiters;
    const bool duals = in.big && interior256 && in.use_glds && (kit % 2 == 0) && BM == 2 * BN;
    p.tiles = tile_list(nrb, ncb, BM, BN, duals, &p.has_duals);
    const int ntiles = (int)p.tiles.size();
    const int64_t total = (int64_t)ntiles * kit;
    int grid = in.big ? in.num_cu : 2 * in.num_cu;
    if (in.grid_cap > 0 && grid > in.grid_cap) grid = in.grid_cap;     // one instance of a batch: its share of the chip
    if (grid > total) grid = (int)total;
    if (grid < ntiles && total / ntiles < 8) { grid = ntiles; p.tiny_k = true; }   // tiny K: one tile per workgroup
    const int64_t per = (total + grid - 1) / grid;
    grid = (int)((total + per - 1) / per);
    p.grid = grid;
    p.per = (int)per;
    // ---- unit ranges per workgroup
    p.ranges.assign((size_t)grid * GRAM_RMAX * 2, 0);
    const int64_t q = kit / per, rem = kit % per;
    // (a tail workgroup crosses at most per/rem + 2 remainders)
    p.aligned = in.big && q >= 1 && rem > 0 && (int64_t)ntiles * q < grid && per / rem + 2 <= GRAM_RMAX;
    p.whole_tiles = !(in.flags & 1) && !p.aligned && in.big && per >= kit && ntiles >= grid && grid % 8 == 0 && grid >= 8;
    if (p.aligned) p.ok = ranges_aligned(p.tiles, p.ranges, grid, per, kit);
    else if (p.whole_tiles) ranges_whole_tiles(p.tiles, p.ranges, grid, kit);
    else {
        ranges_plain(p.ranges, grid, per, total);
        if (in.big) p.xcd_D = xcd_stride_order(p.tiles, nrb, ncb, per, kit);
    }
    if (p.ok) replay_contributors(p);
    return p;
}

// Inverse merge plan: binary tree over the NB-blocks of L (m x m, leading dimension m), W its inverse, T scratch.
// Per level two products: T1 = L21 * W11, then W21 = -W22 * T1.  The 64 x 64-tile kernel is bound by
// the latency of its k-steps, and the top levels have few tiles with long K: products with K >= 512
// are cut into pieces of 256 along K (written to P, m*m doubles; zero ranges of the triangular operands
// skipped per piece) and summed by a reduction launch in a fixed order.
struct MergePlan {
    std::vector<GemmOp> ops;
    std::vector<RedOp> reds;
    std::vector<MergeStage> stages;
};
inline MergePlan plan_merges(int64_t m, const double* L, double* W, double* T, double* P) {
    MergePlan mp;
    const int nblk = (int)((m + NB - 1) / NB);
    for (int span = 1; span < nblk; span *= 2) {
        std::vector<GemmOp> first, second;
        for (int g = 0; g + span < nblk; g += 2 * span) {
            const int64_t r1 = (int64_t)g * NB;                         // left group rows/cols start
            const int64_t s1 = (int64_t)span * NB;                      // left size (always full)
            const int64_t r2 = r1 + s1;
            const int64_t s2 = std::min<int64_t>((int64_t)span * NB, m - r2);
            GemmOp a{};
            a.A = L + r2 * m + r1; a.lda = m;                           // L21 (s2 x s1)
            a.B = W + r1 * m + r1; a.ldb = m;                           // W11 (s1 x s1), B[k][col]
            a.C = T + r2 * m + r1; a.ldc = m;                           // T1  (s2 x s1)
            a.M = (int)s2; a.N = (int)s1; a.K = (int)s1; a.lower_only = 0; a.alpha = 1.0; a.beta = 0.0;
            a.tri = 1;                                                  // W11 is lower triangular
            GemmOp b{};
            b.A = W + r2 * m + r2; b.lda = m;                           // W22 (s2 x s2)
            b.B = T + r2 * m + r1; b.ldb = m;                           // T1, B[k][col]
            b.C = W + r2 * m + r1; b.ldc = m;                           // W21
            b.M = (int)s2; b.N = (int)s1; b.K = (int)s2; b.lower_only = 0; b.alpha = -1.0; b.beta = 0.0;
            b.tri = 2;                                                  // W22 is lower triangular
            first.push_back(a);
            second.push_back(b);
        }
        for (std::vector<GemmOp>* list : {&first, &second}) {
            // split when every product of the list is a whole number of K pieces (full-size groups; N even)
            bool split = !list->empty();
            size_t pdoubles = 0;
            for (const GemmOp& o : *list) {
                split = split && o.K >= KSPLIT_MIN && o.K % KP == 0 && (o.N % 2 == 0) && (o.ldc % 2 == 0);
                pdoubles += (size_t)(o.K / KP) * o.M * o.N;
            }
            split = split && pdoubles <= (size_t)m * m;
            MergeStage st{0, (int)mp.ops.size(), 0, 0, 0};
            MergeStage rs{1, (int)mp.reds.size(), 0, 0, 0};
            double* pb = P;
            for (const GemmOp& o : *list) {
                st.maxm = std::max(st.maxm, o.M); st.maxn = std::max(st.maxn, o.N);
                if (!split) { mp.ops.push_back(o); continue; }
                const int ns = (int)(o.K / KP);
                RedOp r{o.C, pb, o.ldc, o.M, o.N, ns, 0};
                mp.reds.push_back(r);
                rs.maxm = std::max(rs.maxm, o.M * o.N);
                for (int p = 0; p < ns; ++p) {
                    GemmOp q = o;
                    q.A = o.A + p * KP;                                 // A[row][k]: k is the fast index
                    q.B = o.B + p * KP * o.ldb;                         // B[k][col]
                    q.K = (int)KP;
                    q.koff = (int)(p * KP);
                    q.C = pb; q.ldc = o.N;
                    pb += (size_t)o.M * o.N;
                    mp.ops.push_back(q);
                }
            }
            st.end = (int)mp.ops.size();
            mp.stages.push_back(st);
            if (split) { rs.end = (int)mp.reds.size(); mp.stages.push_back(rs); }
        }
    }
    return mp;
}

// One-launch Cholesky over T block columns: a workgroup per tile (the owner of a diagonal tile also owns the tile left
// of it)
inline std::vector<CholJob> chol_jobs(int T) {
    std::vector<CholJob> jobs;
    for (int d2 = 0; d2 < T; ++d2) jobs.push_back(CholJob{d2, d2});            // the chain first
    for (int j = 0; j < T; ++j)                                               // then by urgency: leftmost columns
        for (int i = j + 2; i < T; ++i) jobs.push_back(CholJob{i, j});
    return jobs;
}

}  // namespace accbpg
