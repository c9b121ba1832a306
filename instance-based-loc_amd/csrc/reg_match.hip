// reg_match.hip -- feature stage of a registration pass: normals / FPFH / colour gradients of the job clouds from the instance caches
// or recomputed in the context of their job, 33-d feature matching with mutual filter.
//
// Replaces, for a whole batch of (frame, assignment) jobs at once, the feature and correspondence part of
//   utils/fpfh_register.py:100-143            register_point_clouds (preprocessing + RegistrationRANSACBasedOnFeatureMatching's matching)
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdlib>
#include <map>
#include <vector>

#include "ibloc.h"
#include "reg_common.h"
#include "reg_stages.h"

// ------------------------------------------------------------------------------------------------
// feature stage: recomputed groups (raw concatenations of the instances that influence each other) and the
// assembly of the per-job feature arrays from the instance caches / the recomputed groups
// ------------------------------------------------------------------------------------------------
#define FEATCOPY_GRAD 4                              // also copy the colour gradients (target sides)

__global__ __launch_bounds__(256) void ibl_group_gather_kernel(const GroupDesc* __restrict__ groups, int G, const float4* __restrict__ det,
                                                               const int* __restrict__ det_off, const float4* __restrict__ mem,
                                                               const int* __restrict__ mem_off, const int* __restrict__ grp_off,
                                                               float4* __restrict__ out) {
    const int n = grp_off[G];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int g = seg_of(grp_off, G, i);
    int local = i - grp_off[g];
    const float4* pool = groups[g].pool ? mem : det;
    const int* off = groups[g].pool ? mem_off : det_off;
    float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int t = 0; t < 3; ++t) {
        const int sg = groups[g].seg[t];
        if (sg < 0) continue;
        const int len = off[sg + 1] - off[sg];
        if (local < len) { p = pool[off[sg] + local]; break; }
        local -= len;
    }
    out[i] = p;
}

// Exact form of "instance B is within the influence radius of instance A": is any point of A closer than R to a point of B?
// Bounding boxes alone call most neighbouring instances close (their boxes overlap in empty corners), which forces their
// features to be recomputed in every job that contains both.  grid (NEAR_SPLIT, pairs): every block keeps the points of B
// that lie within R of A's box in LDS and sweeps its share of A's points (those within R of B's box) over them.
#define NEAR_SPLIT 8
#define NEAR_CAP 5120

__device__ __forceinline__ float box_dist2(const float* bx, float x, float y, float z) {
    const float dx = fmaxf(fmaxf(bx[0] - x, x - bx[3]), 0.0f), dy = fmaxf(fmaxf(bx[1] - y, y - bx[4]), 0.0f),
                dz = fmaxf(fmaxf(bx[2] - z, z - bx[5]), 0.0f);
    return dx * dx + dy * dy + dz * dz;
}

__global__ __launch_bounds__(256) void ibl_near_pair_kernel(const NearPair* __restrict__ pairs, const float4* __restrict__ det,
                                                            const int* __restrict__ det_off, const float4* __restrict__ mem,
                                                            const int* __restrict__ mem_off, float R2, int* __restrict__ flags) {
    const NearPair P = pairs[blockIdx.y];
    const float4* pool = P.pool ? mem : det;
    const int* off = P.pool ? mem_off : det_off;
    const int ab = off[P.a], ae = off[P.a + 1], bb = off[P.b], be = off[P.b + 1];
    __shared__ float sx[NEAR_CAP], sy[NEAR_CAP], sz[NEAR_CAP];
    __shared__ int nb, found;
    if (threadIdx.x == 0) { nb = 0; found = 0; }
    __syncthreads();
    for (int i = bb + threadIdx.x; i < be; i += 256) {
        const float4 p = pool[i];
        if (box_dist2(P.boxa, p.x, p.y, p.z) < R2) {
            const int pos = atomicAdd(&nb, 1);
            if (pos < NEAR_CAP) { sx[pos] = p.x; sy[pos] = p.y; sz[pos] = p.z; }
        }
    }
    __syncthreads();
    const int n = nb;
    if (n > NEAR_CAP) { if (threadIdx.x == 0) atomicOr(&flags[blockIdx.y], 1); return; }     // too many to hold: call it close
    if (n == 0) return;
    for (int i0 = ab + blockIdx.x * 256; i0 < ae; i0 += NEAR_SPLIT * 256) {
        const int i = i0 + threadIdx.x;
        bool hit = false;
        if (i < ae) {
            const float4 p = pool[i];
            if (box_dist2(P.boxb, p.x, p.y, p.z) < R2)
                for (int j = 0; j < n; ++j)
                    if (dist2f(p.x, p.y, p.z, sx[j], sy[j], sz[j]) < R2) { hit = true; break; }
        }
        if (hit) found = 1;
        __syncthreads();
        if (found) break;
    }
    if (threadIdx.x == 0 && found) atomicOr(&flags[blockIdx.y], 1);
}

// grid (tiles, copies): contiguous block copies (an instance's features are contiguous at both ends)
__global__ __launch_bounds__(256) void ibl_feat_assemble_kernel(const FeatCopy* __restrict__ copies, FeatSources src, float4* __restrict__ normals,
                                                                float* __restrict__ fpfh, float4* __restrict__ grad) {
    const FeatCopy c = copies[blockIdx.y];
    const int k = c.kind & 3;
    if (fpfh) {
        const float* sf = src.fpfh[k] + (int64_t)c.src * 33;
        float* df = fpfh + (int64_t)c.dst * 33;
        const int nf = c.count * 33;
        for (int i = blockIdx.x * 256 + threadIdx.x; i < nf; i += gridDim.x * 256) df[i] = sf[i];
    }
    const float4* sn = src.normals[k] + c.src;
    const float4* sg = src.grad[k] + c.src;
    const bool want_grad = (c.kind & FEATCOPY_GRAD) != 0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < c.count; i += gridDim.x * 256) {
        normals[c.dst + i] = sn[i];
        if (want_grad) grad[c.dst + i] = sg[i];
    }
}

// ------------------------------------------------------------------------------------------------
// feature matching: 1-NN in 33-d (fp32 fmaf chain over the bins in matching order, first minimum wins), both directions
// grid (tiles, 2J): y < J: queries = source j, database = target j;  y >= J: the reverse
// ------------------------------------------------------------------------------------------------
// A job side is a concatenation of up to three instances, and the same (query instance, database instance) pair recurs in
// many jobs of a frame (every assignment that contains both), so the search runs once per distinct PAIR and a job's
// nearest neighbours are folded from its pairs in concatenation order with a strict '<' -- exactly the first minimum the
// scan over the concatenated database finds.  Features are read in place (instance caches / recomputed groups).
#define FT_TILE 32

// grid (query tiles, pairs)
// INDEXED: only the queries listed for the pair are searched (the target points that are some source point's nearest
// neighbour -- the mutual filter reads no other target's result): need_pos = exclusive scan of the need flags over the
// region of these pairs' outputs (which starts at out0), need_list = the flagged positions in order.
template <bool INDEXED>
__global__ __launch_bounds__(256) void ibl_feat_pair_nn_kernel(const FeatPair* __restrict__ pairs, FeatSources src, int* __restrict__ out_idx,
                                                               float* __restrict__ out_d2, const int* __restrict__ need_pos,
                                                               const int* __restrict__ need_list, int out0) {
    const FeatPair P = pairs[blockIdx.y];
    const int q0 = blockIdx.x * 256;
    int n_q = P.qcnt, l0 = 0;
    if (INDEXED) { l0 = need_pos[P.out - out0]; n_q = need_pos[P.out - out0 + P.qcnt] - l0; }
    if (q0 >= n_q) return;
    const float* __restrict__ qf = src.fpfh[P.qkind] + (int64_t)P.qsrc * 33;
    const float* __restrict__ df = src.fpfh[P.dkind] + (int64_t)P.dsrc * 33;
    const bool valid = q0 + (int)threadIdx.x < n_q;
    const int qv = valid ? q0 + (int)threadIdx.x : n_q - 1;
    const int qi = INDEXED ? need_list[l0 + qv] - (P.out - out0) : qv;          // local index of the query inside its instance
    float f[33];
    {
        const float* s = qf + (int64_t)qi * 33;
#pragma unroll
        for (int k = 0; k < 33; ++k) f[k] = s[k];
    }
    // Database rows go through LDS in tiles of FT_TILE rows (padded to 36 floats so that a row is read with broadcast
    // ds_read_b128), shared by the four waves of the block and double-buffered: the next tile's global loads are issued
    // before the current tile is searched and land in registers meanwhile.  (Reading the rows per wave through the scalar
    // cache instead re-fetched every row from L2 once per wave: 5.7 TB/s of L2 traffic, which bound the kernel.)
    __shared__ __attribute__((aligned(16))) float tiles[2][FT_TILE * 36];
    constexpr int PRE = (FT_TILE * 33 + 255) / 256;
    float pre[PRE];
    auto fetch = [&](int t0) {
        const int nt = min(FT_TILE, P.dcnt - t0) * 33;
        const float* __restrict__ g = df + (int64_t)t0 * 33;
#pragma unroll
        for (int i = 0; i < PRE; ++i) { const int e = threadIdx.x + 256 * i; pre[i] = e < nt ? g[e] : 0.0f; }
    };
    auto stash = [&](float* __restrict__ tile) {
#pragma unroll
        for (int i = 0; i < PRE; ++i) {
            const int e = threadIdx.x + 256 * i;
            if (e < FT_TILE * 33) { const int r = e / 33; tile[r * 36 + (e - r * 33)] = pre[i]; }
        }
    };
    float best = INFINITY;
    int bj = 0;
    fetch(0);
    stash(tiles[0]);
    __syncthreads();
    int cur = 0;
    for (int t0 = 0; t0 < P.dcnt; t0 += FT_TILE, cur ^= 1) {
        const bool more = t0 + FT_TILE < P.dcnt;
        if (more) fetch(t0 + FT_TILE);
        const float* __restrict__ tile = tiles[cur];
        const int nt = min(FT_TILE, P.dcnt - t0);
        for (int t = 0; t < nt; ++t) {
            const float* __restrict__ row = tile + t * 36;
            // Rows are stored in matching order (bins from the histogram centres outwards, FEAT_POS in reg_fpfh.hip), so the
            // chain is k = 0..32 over contiguous memory.  Its partial sums are non-decreasing: a target is abandoned as soon
            // as no lane of the wave can still beat its running minimum (checked after 4, 8, 12, 16 and 24 terms); the
            // surviving distances are the complete chains, bit-identical to the unpruned form.
            float acc = 0.0f;
#define FT_STAGE(k0, k1)                                                                                       \
            _Pragma("unroll") for (int k = k0; k < k1; ++k) { const float d = f[k] - row[k]; acc = __builtin_fmaf(d, d, acc); }
            FT_STAGE(0, 4)
            if (__ballot(acc < best) == 0ull) continue;
            FT_STAGE(4, 8)
            if (__ballot(acc < best) == 0ull) continue;
            FT_STAGE(8, 12)
            if (__ballot(acc < best) == 0ull) continue;
            FT_STAGE(12, 16)
            if (__ballot(acc < best) == 0ull) continue;
            FT_STAGE(16, 24)
            if (__ballot(acc < best) == 0ull) continue;
            FT_STAGE(24, 33)
#undef FT_STAGE
            if (acc < best) { best = acc; bj = t0 + t; }
        }
        if (more) stash(tiles[cur ^ 1]);
        __syncthreads();
    }
    if (valid) { out_idx[P.out + qi] = bj; out_d2[P.out + qi] = best; }
}

// thread per point of every job side: fold the pair results of its instance over the database instances in order
__global__ __launch_bounds__(256) void ibl_feat_fold_kernel(const SidePairs* __restrict__ sides, const FeatPair* __restrict__ pairs,
                                                            const int* __restrict__ pair_idx, const float* __restrict__ pair_d2,
                                                            const int* __restrict__ job_off, int J, int i0, int i1, int* __restrict__ nn) {
    const int i = i0 + blockIdx.x * 256 + threadIdx.x;
    if (i >= i1) return;
    const int sgi = seg_of(job_off, 2 * J, i);
    const SidePairs S = sides[sgi];
    int local = i - job_off[sgi], a = 0;
    while (a < 2 && local >= S.qcnt[a]) { local -= S.qcnt[a]; ++a; }
    float best = INFINITY;
    int bj = 0, dbase = 0;
    for (int b = 0; b < 3; ++b) {
        const int p = S.pair[a][b];
        if (p >= 0) {
            const int o = pairs[p].out + local;
            const float d = pair_d2[o];
            if (d < best) { best = d; bj = dbase + pair_idx[o]; }
        }
        dbase += S.dcnt[b];
    }
    nn[i] = bj;
}

// thread per source point: flag the target point it matched as needed in every (target instance -> source instance) pair of
// its job (the target's own nearest neighbour is folded over all source instances of the job)
__global__ __launch_bounds__(256) void ibl_feat_need_kernel(const SidePairs* __restrict__ sides, const FeatPair* __restrict__ pairs,
                                                            const int* __restrict__ job_off, int J, const int* __restrict__ nn, int out0,
                                                            int* __restrict__ need) {
    const int ns = job_off[J];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= ns) return;
    const int j = seg_of(job_off, J, i);
    const SidePairs S = sides[j];                 // source side: dcnt = sizes of the target instances
    int local = nn[i], b = 0;
    if (local >= S.dcnt[0] + S.dcnt[1] + S.dcnt[2]) return;        // empty target side
    while (b < 2 && local >= S.dcnt[b]) { local -= S.dcnt[b]; ++b; }
    const SidePairs T = sides[J + j];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int p = T.pair[b][a];
        if (p >= 0) need[pairs[p].out - out0 + local] = 1;
    }
}

__global__ __launch_bounds__(256) void ibl_feat_need_list_kernel(const int* __restrict__ need, const int* __restrict__ pos, int n,
                                                                 int* __restrict__ list) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < n && need[e]) list[pos[e]] = e;
}

// one block per job: mutual filter + ordered compaction; falls back to all source->target matches when fewer than
// 3 * ransac_n survive (Open3D RegistrationRANSACBasedOnFeatureMatching)
__global__ __launch_bounds__(256) void ibl_mutual_kernel(const int* __restrict__ nn, const int* __restrict__ job_off, int J, int mutual,
                                                         int min_mutual, int2* __restrict__ corr /* capacity: source offsets */,
                                                         int* __restrict__ n_corr) {
    const int j = blockIdx.x;
    const int sb = job_off[j], se = job_off[j + 1], tb = job_off[J + j], te = job_off[J + j + 1];
    const int ns = se - sb, nt = te - tb;
    __shared__ int wave_cnt[4];
    __shared__ int base;
    if (threadIdx.x == 0) base = 0;
    __syncthreads();
    if (ns == 0 || nt == 0) { if (threadIdx.x == 0) n_corr[j] = 0; return; }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (mutual) {
        for (int i0 = 0; i0 < ns; i0 += 256) {
            const int i = i0 + threadIdx.x;
            bool keep = false;
            int tj = 0;
            if (i < ns) { tj = nn[sb + i]; keep = nn[tb + tj] == i; }
            const unsigned long long m = __ballot(keep);
            if (lane == 0) wave_cnt[wave] = __popcll(m);
            __syncthreads();
            int pre = base;
            for (int w = 0; w < wave; ++w) pre += wave_cnt[w];
            if (keep) corr[sb + pre + __popcll(m & ((1ull << lane) - 1ull))] = make_int2(i, tj);
            __syncthreads();
            if (threadIdx.x == 0) base += wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
            __syncthreads();
        }
        if (base >= min_mutual) { if (threadIdx.x == 0) n_corr[j] = base; return; }
    }
    for (int i = threadIdx.x; i < ns; i += 256) corr[sb + i] = make_int2(i, nn[sb + i]);
    if (threadIdx.x == 0) n_corr[j] = ns;
}

// ------------------------------------------------------------------------------------------------
// host plan (no device, no context): which instances keep their stand-alone features, which searches run
// ------------------------------------------------------------------------------------------------
static double box_gap2(const float* ba, const float* bb) {
    double g2 = 0;
    for (int c = 0; c < 3; ++c) {
        const double gap = std::max(0.0, std::max((double)ba[c] - (double)bb[3 + c], (double)bb[c] - (double)ba[3 + c]));
        g2 += gap * gap;
    }
    return g2;
}

// instances of one job side whose boxes are within R: the candidates of the exact (point set) test on the device
static void list_near_candidates(const HostTables& h, double R, MatchPlan* plan) {
    for (int sgi = 0; sgi < 2 * h.J; ++sgi) {
        const int pl = sgi >= h.J ? 1 : 0, j = pl ? sgi - h.J : sgi;
        if (!h.bbox[pl]) continue;
        const int* segs = pl ? h.jobs[j].tgt_seg : h.jobs[j].src_seg;
        for (int a = 0; a < 3; ++a)
            for (int b = a + 1; b < 3; ++b) {
                if (segs[a] < 0 || segs[b] < 0) continue;
                const std::array<int, 3> key = {pl, std::min(segs[a], segs[b]), std::max(segs[a], segs[b])};
                const float *ba = h.bbox[pl] + 6 * (size_t)key[1], *bb = h.bbox[pl] + 6 * (size_t)key[2];
                if (plan->near_id.count(key) || box_gap2(ba, bb) >= R * R) continue;
                NearPair np;
                np.pool = pl; np.a = key[1]; np.b = key[2]; np.pad = 0;
                for (int c = 0; c < 6; ++c) { np.boxa[c] = ba[c]; np.boxb[c] = bb[c]; }
                plan->near_id[key] = (int)plan->near.size();
                plan->near.push_back(np);
            }
    }
    plan->near_flag.assign(plan->near.size(), 0);
}

// Which instances of every job side keep their stand-alone features: an instance is dirty when another instance of its side is
// within the influence radius (near_flag) or when its pool has no instance features.  The dirty instances of a side form a
// recomputed group (shared between the sides that have the same one).  -> slots, groups, grp_off, copies, reuse_stats[0..3]
static void plan_feature_reuse(const HostTables& h, MatchPlan* plan) {
    std::map<std::array<int, 4>, int> gid[2];
    std::vector<std::array<int, 4>> gkeys[2];
    std::vector<SlotPlan>& slots = plan->slots;
    slots.reserve((size_t)6 * h.J);
    int64_t pts_cached = 0;
    for (int sgi = 0; sgi < 2 * h.J; ++sgi) {
        const int pl = sgi >= h.J ? 1 : 0, j = pl ? sgi - h.J : sgi;
        const int* segs = pl ? h.jobs[j].tgt_seg : h.jobs[j].src_seg;
        const int* off = h.off[pl];
        bool dirty[3] = {false, false, false};
        for (int a = 0; a < 3; ++a) {
            if (segs[a] < 0) continue;
            if (!h.bbox[pl]) { dirty[a] = true; continue; }
            for (int b = 0; b < 3; ++b) {
                if (b == a || segs[b] < 0) continue;
                const auto it = plan->near_id.find({pl, std::min(segs[a], segs[b]), std::max(segs[a], segs[b])});
                if (it != plan->near_id.end() && plan->near_flag[it->second]) dirty[a] = true;
            }
        }
        std::array<int, 4> key = {pl, -1, -1, -1};
        int nd = 0, pos[3] = {0, 0, 0}, acc = 0;
        for (int a = 0; a < 3; ++a)
            if (segs[a] >= 0 && dirty[a]) { key[1 + nd++] = segs[a]; pos[a] = acc; acc += off[segs[a] + 1] - off[segs[a]]; }
        int g = -1;
        if (nd > 0) {
            auto it = gid[pl].find(key);
            if (it == gid[pl].end()) { g = (int)gkeys[pl].size(); gid[pl][key] = g; gkeys[pl].push_back(key); }
            else g = it->second;
        }
        int dst = h.job_off[sgi];
        for (int a = 0; a < 3; ++a) {
            if (segs[a] < 0) continue;
            const int cnt = off[segs[a] + 1] - off[segs[a]];
            slots.push_back({dst, cnt, pl, segs[a], dirty[a] ? g : -1, pos[a], sgi, 0, 0});
            if (!dirty[a]) pts_cached += cnt;
            dst += cnt;
        }
    }
    // recomputed groups: detected-pool groups first, memory-pool groups last (their points get colour gradients)
    const int G0 = (int)gkeys[0].size(), G = G0 + (int)gkeys[1].size();
    plan->G0 = G0;
    plan->groups.resize(G);
    plan->grp_off.assign(G + 1, 0);
    for (int g = 0; g < G; ++g) {
        const std::array<int, 4>& k = g < G0 ? gkeys[0][g] : gkeys[1][g - G0];
        const int* off = h.off[k[0]];
        plan->groups[g].pool = k[0];
        int cnt = 0;
        for (int t = 0; t < 3; ++t) { plan->groups[g].seg[t] = k[1 + t]; if (k[1 + t] >= 0) cnt += off[k[1 + t] + 1] - off[k[1 + t]]; }
        plan->grp_off[g + 1] = plan->grp_off[g] + cnt;
    }
    plan->reuse_stats[0] = pts_cached; plan->reuse_stats[1] = plan->grp_off[G]; plan->reuse_stats[2] = G; plan->reuse_stats[3] = 2 * h.J;
    plan->copies.reserve(slots.size());
    for (SlotPlan& sp : slots) {
        if (sp.grp < 0) { sp.kind = sp.pool; sp.src = h.off[sp.pool][sp.seg]; }
        else { sp.kind = 2; sp.src = plan->grp_off[(sp.pool ? G0 : 0) + sp.grp] + sp.pos; }
        if (sp.count <= 0) continue;
        FeatCopy c;
        c.dst = sp.dst; c.count = sp.count; c.kind = sp.kind; c.src = sp.src;
        if (sp.pool == 1) c.kind |= FEATCOPY_GRAD;
        plan->copies.push_back(c);
    }
}

// feature matching plan: the distinct (query instance, database instance) pairs -> pairs, sides, pts0, n_pairs0, max_q,
// reuse_stats[4..5]
static int plan_feature_pairs(const HostTables& h, MatchPlan* plan) {
    const int J = h.J;
    const std::vector<SlotPlan>& slots = plan->slots;
    std::vector<FeatPair>& pairs = plan->pairs;
    std::vector<int> side_first(2 * J + 1, 0);      // slots are stored side by side, in slot order
    for (const SlotPlan& sp : slots) ++side_first[sp.side + 1];
    for (int i = 0; i < 2 * J; ++i) side_first[i + 1] += side_first[i];
    std::map<std::array<int, 4>, int> pid;
    plan->sides.assign(2 * J, SidePairs{});
    int64_t pair_pts = 0;     // outputs of the source-query pairs come first: [0, pts0)
    for (int sgi = 0; sgi < 2 * J; ++sgi) {
        if (sgi == J) { plan->pts0 = pair_pts; plan->n_pairs0 = (int)pairs.size(); }
        const int other = sgi < J ? sgi + J : sgi - J;
        SidePairs& S = plan->sides[sgi];
        for (int a = 0; a < 3; ++a) { S.qcnt[a] = S.dcnt[a] = 0; for (int b = 0; b < 3; ++b) S.pair[a][b] = -1; }
        const int nq = side_first[sgi + 1] - side_first[sgi], nd = side_first[other + 1] - side_first[other];
        for (int a = 0; a < nq; ++a) S.qcnt[a] = slots[side_first[sgi] + a].count;
        for (int b = 0; b < nd; ++b) S.dcnt[b] = slots[side_first[other] + b].count;
        for (int a = 0; a < nq; ++a)
            for (int b = 0; b < nd; ++b) {
                const SlotPlan& q = slots[side_first[sgi] + a];
                const SlotPlan& d = slots[side_first[other] + b];
                if (q.count <= 0 || d.count <= 0) continue;
                const std::array<int, 4> key = {q.kind, q.src, d.kind, d.src};
                auto it = pid.find(key);
                int id;
                if (it == pid.end()) {
                    if (pair_pts + q.count > 0x7fffffff) return ibl_set_error(IBL_ERR_OVERFLOW, "feature matching: pair table exceeds 2^31 entries");
                    id = (int)pairs.size();
                    pid[key] = id;
                    pairs.push_back({q.kind, q.src, q.count, d.kind, d.src, d.count, (int)pair_pts, 0});
                    pair_pts += q.count;
                    plan->max_q = std::max(plan->max_q, q.count);
                } else id = it->second;
                S.pair[a][b] = id;
            }
    }
    plan->pair_pts = pair_pts;
    int64_t uses = 0;
    for (const SidePairs& S : plan->sides)
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) uses += S.pair[a][b] >= 0 ? 1 : 0;
    plan->reuse_stats[4] = (int64_t)pairs.size();
    plan->reuse_stats[5] = uses;
    return IBL_OK;
}

// A group's bounding box is the union of its instances' boxes (the gathered points are theirs, untouched), which the host holds
// with the instance features: the group grids are dimensioned without a read-back.  Empty: a pool without instance features.
static std::vector<float> group_boxes(const HostTables& h, const MatchPlan& plan) {
    std::vector<float> grp_bbox;
    for (const GroupDesc& g : plan.groups)
        if (!h.bbox[g.pool]) return grp_bbox;
    grp_bbox.resize(plan.groups.size() * 6);
    for (size_t g = 0; g < plan.groups.size(); ++g) {
        const GroupDesc& gd = plan.groups[g];
        union_of_boxes(gd.seg, -1, h.off[gd.pool], h.bbox[gd.pool], &grp_bbox[6 * g], &grp_bbox[6 * g + 3]);
    }
    return grp_bbox;
}

// ------------------------------------------------------------------------------------------------
// the device half
// ------------------------------------------------------------------------------------------------
struct MatchDev { int* nn; SidePairs* d_sides; FeatPair* d_pairs; int* pair_idx; float* pair_d2; };

static int check_instance_features(const RegCall& c, double grad_radius) {
    const ibl_instance_features* feat[2] = {c.det.features, c.mem.features};
    for (int pl = 0; pl < 2; ++pl) {
        if (!feat[pl]) continue;
        if (!feat[pl]->normals4 || !feat[pl]->fpfh || !feat[pl]->fpfh_norm || !feat[pl]->bbox)       // (fpfh_split may be null: compact features)
            return ibl_set_error(IBL_ERR_ARG, "ibl_register_jobs: instance features with null arrays");
        if (fabs(feat[pl]->voxel_size - c.params.voxel_size) > 1e-12 * c.params.voxel_size)
            return ibl_set_error(IBL_ERR_ARG, "ibl_register_jobs: instance features were built for voxel_size %g, not %g",
                                 feat[pl]->voxel_size, c.params.voxel_size);
        if (pl == 1 && (!feat[pl]->grad4 || fabs(feat[pl]->grad_radius - grad_radius) > 1e-12 * grad_radius))
            return ibl_set_error(IBL_ERR_ARG, "ibl_register_jobs: memory features need colour gradients of radius %g "
                                 "(2 * voxel_size * local_dist_factor)", grad_radius);
    }
    return IBL_OK;
}

// decides the near pairs exactly (point sets) -> plan.near_flag, read back
static int test_near_pairs(ibl_reg_ctx* ctx, RegPass& ps, double R) {
    std::vector<NearPair>& near = ps.plan.near;
    if (near.empty()) return IBL_OK;
    hipStream_t s = ps.s;
    ArenaMark mn(ctx);
    NearPair* d_near; int* d_flags;
    IBL_ARENA(d_near, NearPair, (int64_t)near.size());
    IBL_ARENA(d_flags, int, (int64_t)near.size());
    const int st = ibl_stage_upload(ctx, d_near, near.data(), sizeof(NearPair) * (int64_t)near.size(), s);
    if (st) return st;
    IBL_HIP_CHECK(hipMemsetAsync(d_flags, 0, sizeof(int) * near.size(), s));
    const float Rf = nextafterf((float)R, INFINITY);
    for (size_t p0 = 0; p0 < near.size(); p0 += 32768) {
        const unsigned np = (unsigned)std::min<size_t>(32768, near.size() - p0);
        hipLaunchKernelGGL(ibl_near_pair_kernel, dim3(NEAR_SPLIT, np), dim3(256), 0, s, d_near + p0, ps.det, ps.call->det.off_dev, ps.mem,
                           ps.call->mem.off_dev, Rf * Rf * 1.000001f, d_flags + p0);
        IBL_LAUNCH_CHECK();
    }
    IBL_HIP_CHECK(hipMemcpyAsync(ps.plan.near_flag.data(), d_flags, sizeof(int) * near.size(), hipMemcpyDeviceToHost, s));
    IBL_HIP_CHECK(hipStreamSynchronize(s));
    return IBL_OK;
}

// gathers the recomputed groups and computes their features -> src [2]; the scratch belongs to the caller's arena mark
static int recompute_groups(ibl_reg_ctx* ctx, RegPass& ps, const HostTables& h, double grad_radius, FeatSources* src) {
    const MatchPlan& plan = ps.plan;
    const RegCall& c = *ps.call;
    hipStream_t s = ps.s;
    const int G = (int)plan.groups.size(), Nd = plan.grp_off[G];
    GroupDesc* d_groups; int* d_grp_off; float4 *Pd, *normals_d, *grad_d; float *fpfh_d, *norm_d; unsigned short* split_d;
    IBL_ARENA(d_groups, GroupDesc, G);
    IBL_ARENA(d_grp_off, int, G + 1);
    IBL_ARENA(Pd, float4, Nd + 1);
    IBL_ARENA(normals_d, float4, Nd + 1);
    IBL_ARENA(grad_d, float4, Nd + 1);
    IBL_ARENA(fpfh_d, float, (int64_t)Nd * 33 + 64);
    IBL_ARENA(split_d, unsigned short, (int64_t)Nd * 48 + 64);
    IBL_ARENA(norm_d, float, (int64_t)Nd + 64);
    int st = ibl_stage_upload(ctx, d_groups, plan.groups.data(), sizeof(GroupDesc) * (int64_t)G, s);
    if (st) return st;
    st = ibl_stage_upload(ctx, d_grp_off, plan.grp_off.data(), sizeof(int) * (int64_t)(G + 1), s);
    if (st) return st;
    hipLaunchKernelGGL(ibl_group_gather_kernel, dim3((Nd + 255) / 256), dim3(256), 0, s, d_groups, G, ps.det, c.det.off_dev, ps.mem,
                       c.mem.off_dev, d_grp_off, Pd);
    IBL_LAUNCH_CHECK();
    const std::vector<float> grp_bbox = group_boxes(h, plan);
    st = ibl_features_on_batch(ctx, Pd, d_grp_off, plan.grp_off.data(), G, grp_bbox.empty() ? nullptr : grp_bbox.data(), c.params.voxel_size, grad_radius,
                               plan.grp_off[plan.G0], Nd, normals_d, fpfh_d, split_d, norm_d, grad_d, s);
    if (st) return st;
    src->normals[2] = normals_d; src->fpfh[2] = fpfh_d; src->grad[2] = grad_d; src->split[2] = split_d; src->norm[2] = norm_d;
    return IBL_OK;
}

// normals (and the target sides' colour gradients) of the job clouds from the instance caches / the recomputed groups
static int assemble_features(ibl_reg_ctx* ctx, RegPass& ps, const FeatSources& src) {
    const std::vector<FeatCopy>& copies = ps.plan.copies;
    FeatCopy* d_copies;
    IBL_ARENA(d_copies, FeatCopy, (int64_t)copies.size());
    const int st = ibl_stage_upload(ctx, d_copies, copies.data(), sizeof(FeatCopy) * (int64_t)copies.size(), ps.s);
    if (st) return st;
    for (size_t c0 = 0; c0 < copies.size(); c0 += 32768) {
        const unsigned nc = (unsigned)std::min<size_t>(32768, copies.size() - c0);
        hipLaunchKernelGGL(ibl_feat_assemble_kernel, dim3(8, nc), dim3(256), 0, ps.s, d_copies + c0, src, ps.normals, (float*)nullptr, ps.grad);
        IBL_LAUNCH_CHECK();
    }
    return IBL_OK;
}

// (2) of search_features: the reverse search only for the target points that were matched (a third to a half of them): flag, scan,
//     list, search the listed queries; the other targets keep d2 = +inf and are never read
static int search_needed_targets(ibl_reg_ctx* ctx, RegPass& ps, const FeatSources& src, const MatchDev& d, bool use_mfma) {
    const MatchPlan& plan = ps.plan;
    hipStream_t s = ps.s;
    const int J = ps.J, Ns = ps.Ns, n_pairs0 = plan.n_pairs0, max_q = plan.max_q;
    const int64_t pts0 = plan.pts0;
    const int n1 = (int)(plan.pair_pts - pts0);
    const int n_pairs1 = (int)plan.pairs.size() - n_pairs0;
    if (!(n1 > 0 && n_pairs1 > 0 && Ns > 0)) return IBL_OK;
    int *need, *need_pos, *need_list;
    IBL_ARENA(need, int, (int64_t)n1 + 1);
    IBL_ARENA(need_pos, int, (int64_t)n1 + 1);
    IBL_ARENA(need_list, int, (int64_t)n1 + 1);
    IBL_HIP_CHECK(hipMemsetAsync(need, 0, sizeof(int) * ((size_t)n1 + 1), s));
    IBL_HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)(d.pair_d2 + pts0), 0x7f800000, (size_t)n1, s));
    IBL_HIP_CHECK(hipMemsetAsync(d.pair_idx + pts0, 0, sizeof(int) * (size_t)n1, s));
    hipLaunchKernelGGL(ibl_feat_need_kernel, dim3((Ns + 255) / 256), dim3(256), 0, s, d.d_sides, d.d_pairs, ps.d_job_off, J, d.nn, (int)pts0, need);
    IBL_LAUNCH_CHECK();
    size_t tmp_bytes = 0;
    IBL_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, need, need_pos, n1 + 1, s));
    unsigned char* tmp;
    IBL_ARENA(tmp, unsigned char, (int64_t)tmp_bytes + 256);
    IBL_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, need, need_pos, n1 + 1, s));
    hipLaunchKernelGGL(ibl_feat_need_list_kernel, dim3((n1 + 255) / 256), dim3(256), 0, s, need, need_pos, n1, need_list);
    IBL_LAUNCH_CHECK();
    ps.dbg("need list");
    bool over = !use_mfma;
    if (use_mfma) {
        const int st = ibl_feat_search_mfma(ctx, d.d_pairs + n_pairs0, n_pairs1, max_q, src, d.pair_idx, d.pair_d2, need_pos, need_list, (int)pts0, n1,
                                            &over, s);
        if (st) return st;
    }
    for (int p0 = 0; over && p0 < n_pairs1; p0 += 32768) {
        const unsigned np = (unsigned)std::min(32768, n_pairs1 - p0);
        hipLaunchKernelGGL(ibl_feat_pair_nn_kernel<true>, dim3((max_q + 255) / 256, np), dim3(256), 0, s, d.d_pairs + n_pairs0 + p0, src,
                           d.pair_idx, d.pair_d2, need_pos, need_list, (int)pts0);
        IBL_LAUNCH_CHECK();
    }
    return IBL_OK;
}

// matching reads the features in place (caches / recomputed groups), once per distinct pair -> d.nn
static int search_features(ibl_reg_ctx* ctx, RegPass& ps, const FeatSources& src, const MatchDev& d) {
    const MatchPlan& plan = ps.plan;
    hipStream_t s = ps.s;
    const int J = ps.J, N = ps.N, Ns = ps.Ns, n_pairs0 = plan.n_pairs0, max_q = plan.max_q;
    int st = ibl_stage_upload(ctx, d.d_sides, plan.sides.data(), sizeof(SidePairs) * (int64_t)plan.sides.size(), s);
    if (st) return st;
    if (plan.pairs.empty() || N <= 0) {
        if (N > 0) IBL_HIP_CHECK(hipMemsetAsync(d.nn, 0, sizeof(int) * (size_t)N, s));
        return IBL_OK;
    }
    st = ibl_stage_upload(ctx, d.d_pairs, plan.pairs.data(), sizeof(FeatPair) * (int64_t)plan.pairs.size(), s);
    if (st) return st;
    // (1) every source point's nearest target: source-query pairs, folded per job
    // matrix-core filter + exact recheck (reg_featnn.hip); the VALU search only if its candidate list overflowed
    const bool use_mfma = !ctx->diag.feat_valu && !ps.opt.force_valu;      // (diagnostics: the tests compare both searches)
    bool over = !use_mfma;
    ps.dbg("plan uploads");
    if (use_mfma) {
        st = ibl_feat_search_mfma(ctx, d.d_pairs, n_pairs0, max_q, src, d.pair_idx, d.pair_d2, nullptr, nullptr, 0, plan.pts0, &over, s);
        if (st) return st;
    }
    ps.dbg("forward search");
    for (int p0 = 0; over && p0 < n_pairs0; p0 += 32768) {
        const unsigned np = (unsigned)std::min(32768, n_pairs0 - p0);
        hipLaunchKernelGGL(ibl_feat_pair_nn_kernel<false>, dim3((max_q + 255) / 256, np), dim3(256), 0, s, d.d_pairs + p0, src, d.pair_idx,
                           d.pair_d2, (const int*)nullptr, (const int*)nullptr, 0);
        IBL_LAUNCH_CHECK();
    }
    if (Ns > 0) {
        hipLaunchKernelGGL(ibl_feat_fold_kernel, dim3((Ns + 255) / 256), dim3(256), 0, s, d.d_sides, d.d_pairs, d.pair_idx, d.pair_d2, ps.d_job_off,
                           J, 0, Ns, d.nn);
        IBL_LAUNCH_CHECK();
    }
    ps.dbg("forward fold");
    st = search_needed_targets(ctx, ps, src, d, use_mfma);
    if (st) return st;
    ps.dbg("reverse search");
    if (N > Ns) {
        hipLaunchKernelGGL(ibl_feat_fold_kernel, dim3((N - Ns + 255) / 256), dim3(256), 0, s, d.d_sides, d.d_pairs, d.pair_idx, d.pair_d2, ps.d_job_off,
                           J, Ns, N, d.nn);
        IBL_LAUNCH_CHECK();
    }
    ps.dbg("reverse fold");
    return IBL_OK;
}

// recomputed groups, assembly of the job clouds' normals / gradients, both searches; its scratch is released on return
// (and reused by later kernels of the same stream only: no synchronisation)
static int features_and_search(ibl_reg_ctx* ctx, RegPass& ps, const HostTables& h, double grad_radius, const MatchDev& d) {
    const RegCall& c = *ps.call;
    ArenaMark md(ctx);
    FeatSources src{};
    const ibl_instance_features* feat[2] = {c.det.features, c.mem.features};
    for (int pl = 0; pl < 2; ++pl)
        if (feat[pl]) {
            src.normals[pl] = reinterpret_cast<const float4*>(feat[pl]->normals4);
            src.fpfh[pl] = feat[pl]->fpfh;
            src.split[pl] = feat[pl]->fpfh_split;
            src.norm[pl] = feat[pl]->fpfh_norm;
            src.grad[pl] = reinterpret_cast<const float4*>(feat[pl]->grad4);
        }
    int st;
    if (ps.plan.grp_off.back() > 0) {
        st = recompute_groups(ctx, ps, h, grad_radius, &src);
        if (st) return st;
    }
    if (!ps.plan.copies.empty()) {
        st = assemble_features(ctx, ps, src);
        if (st) return st;
    }
    ps.phase("recomputed groups + assemble");
    double fl = 0;
    for (int j = 0; j < ps.J; ++j)
        fl += 4.0 * 33.0 * (double)(ps.job_off[j + 1] - ps.job_off[j]) * (double)(ps.job_off[ps.J + j + 1] - ps.job_off[ps.J + j]);
    ibl_prof_begin(IBL_PROF_ST_FEATMATCH, fl, ps.s, &ps.tok_match);
    return search_features(ctx, ps, src, d);
}

// normals + FPFH + colour gradients (instance cache / recomputed groups), then matching -> ps.normals, ps.grad, ps.corr, ps.n_corr
int ibl_reg_match_stage(ibl_reg_ctx* ctx, RegPass& ps) {
    const RegCall& c = *ps.call;
    MatchPlan& plan = ps.plan;
    ArenaMark m2(ctx);
    MatchDev d = {};
    IBL_ARENA(d.nn, int, ps.N + 64);
    const double grad_radius = ps.max_dist_icp * 2.0;
    int st = check_instance_features(c, grad_radius);
    if (st) return st;
    const HostTables h = {ps.J, ps.jobs.data(), ps.job_off.data(), {c.det.off_host, c.mem.off_host},
                          {c.det.features ? c.det.features->bbox : nullptr, c.mem.features ? c.mem.features->bbox : nullptr}};
    // influence radius of a foreign point on the features of an instance (see ibloc.h) + rounding margin
    const double rn = c.params.voxel_size * 2, rf = c.params.voxel_size * 5;
    const double R = std::max(2 * rf + rn, grad_radius + rn) * 1.001 + 1e-4;
    list_near_candidates(h, R, &plan);
    st = test_near_pairs(ctx, ps, R);
    if (st) return st;
    ps.phase("near-pair test");
    plan_feature_reuse(h, &plan);
    if (c.out.reuse_stats) for (int i = 0; i < 4; ++i) c.out.reuse_stats[i] = plan.reuse_stats[i];
    st = plan_feature_pairs(h, &plan);
    if (st) return st;
    if (c.out.reuse_stats) for (int i = 4; i < 6; ++i) c.out.reuse_stats[i] = plan.reuse_stats[i];
    ps.phase("host plan");
    IBL_ARENA(d.d_sides, SidePairs, 2 * ps.J);
    IBL_ARENA(d.d_pairs, FeatPair, (int64_t)plan.pairs.size() + 1);
    IBL_ARENA(d.pair_idx, int, plan.pair_pts + 64);
    IBL_ARENA(d.pair_d2, float, plan.pair_pts + 64);
    st = features_and_search(ctx, ps, h, grad_radius, d);
    if (st) return st;
    ibl_prof_end(ps.tok_match, ps.s);
    ps.phase("feature search");
    hipLaunchKernelGGL(ibl_mutual_kernel, dim3(ps.J), dim3(256), 0, ps.s, d.nn, ps.d_job_off, ps.J, 1, 9, ps.corr, ps.n_corr);
    IBL_LAUNCH_CHECK();
    return IBL_OK;
}
