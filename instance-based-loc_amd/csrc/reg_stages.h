// reg_stages.h -- internals of the registration driver: the call as the C-ABI passes it in, the tables the stages share, and the stage
// functions of one pass (reg_register.hip: job assembly, grid C, read-back; reg_match.hip: features + matching; reg_ransac.hip;
// reg_icp.hip).  reg_eval.hip (whole-memory evaluation, information matrix; the grid itself is reg_memgrid.h / .hip) shares only ICP_BPJ.
#pragma once
#include <algorithm>
#include <array>
#include <map>
#include <vector>

#include "ibloc.h"
#include "reg_common.h"

#define ICP_BPJ 8        // blocks per job in the ICP / evaluation reductions (each ends in a 29-value fp64 block reduction)

// ---- the call -------------------------------------------------------------------------------------
// Arguments of ibl_register_jobs: the public structs of include/ibloc.h (which describes them) by value, the job arrays and the stream.
struct RegCall {
    ibl_cloud_pool det, mem;
    const int32_t* job_src_seg; const int32_t* job_tgt_seg;
    const uint32_t* job_ids;          // host array, one Philox counter word per job, or null: params.job_id_base + j
    int n_jobs;
    ibl_register_params params;
    ibl_register_out out;
    hipStream_t stream;
};
// Choices of one pass: a call is redone with these set after a list overflowed (register_call)
struct RegPassOpts {
    bool force_valu = false;           // VALU feature search: the matrix-core search overflowed its candidate list
    bool ransac_full_list = false;     // survivor list that holds every hypothesis of a round: a RANSAC round overflowed the short one
};

// ---- tables shared by host and device ---------------------------------------------------------------
struct JobDesc {             // host-built, copied to the device
    int src_seg[3];          // segments of the detected pool (-1 = unused)
    int tgt_seg[3];          // segments of the memory pool
};
struct GroupDesc { int pool; int seg[3]; };          // pool 0 = detected, 1 = memory; -1 = unused slot
struct FeatCopy { int dst, src, count, kind; };      // kind & 3: 0 detected cache, 1 memory cache, 2 recomputed groups
struct NearPair { int pool, a, b, pad; float boxa[6], boxb[6]; };
struct SidePairs { int qcnt[3]; int dcnt[3]; int pair[3][3]; };              // per job side: slot sizes, pair ids (-1 = none)

struct RansacState {
    double best_T[16];
    double best_fit, best_rmse;
    long long est_k, next_i, walked, validated, last_update;
    int best_inl;
    int done;
    unsigned job_id;          // the Philox counter word of this job: job_id_base + slot, or the caller's own id (job_ids of ibl_register_jobs)
    int pad_;
};
struct IcpState {
    double T[16];
    double fitness, rmse;
    int iter, done, started;
};

// ---- host plan of the feature stage (reg_match.hip) ---------------------------------------------------
// what the planners read: the job table and, per pool (0 = detected, 1 = memory), the host offsets and the instance boxes
// (bbox[pl] = null: no instance features for that pool, every instance of it is recomputed)
struct HostTables { int J; const JobDesc* jobs; const int* job_off; const int* off[2]; const float* bbox[2]; };
struct SlotPlan { int dst, count, pool, seg, grp, pos, side, kind, src; };       // one instance of one job side
struct MatchPlan {
    std::vector<NearPair> near;                          // instance pairs of one job side whose boxes are within the influence radius
    std::map<std::array<int, 3>, int> near_id;           // (pool, lower segment, higher segment) -> index in near
    std::vector<int> near_flag;                          // the device's exact verdict per near pair
    std::vector<SlotPlan> slots;                         // side by side, in slot order
    std::vector<GroupDesc> groups;                       // recomputed groups: the detected pool's first (G0 of them)
    std::vector<int> grp_off;
    int G0 = 0;
    std::vector<FeatCopy> copies;
    std::vector<FeatPair> pairs;                         // distinct searches: the n_pairs0 source-query pairs first, outputs [0, pts0)
    std::vector<SidePairs> sides;
    int64_t pair_pts = 0, pts0 = 0;
    int n_pairs0 = 0, max_q = 1;
    int64_t reuse_stats[6] = {0, 0, 0, 0, 0, 0};         // ibl_register_out::reuse_stats
};

// union of the boxes ([6] = min xyz, max xyz) of the non-empty instances among segs[0..3) (only >= 0: that slot alone); zeros if none
// (an empty instance's stored box is zeros)
static inline void union_of_boxes(const int* segs, int only, const int* off, const float* boxes, float* lo, float* hi) {
    bool any = false;
    for (int c = 0; c < 3; ++c) lo[c] = hi[c] = 0.0f;
    for (int t = 0; t < 3; ++t) {
        if (only >= 0 && t != only) continue;
        if (segs[t] < 0 || off[segs[t] + 1] == off[segs[t]]) continue;
        const float* b = boxes + 6 * (size_t)segs[t];
        for (int c = 0; c < 3; ++c) { lo[c] = any ? std::min(lo[c], b[c]) : b[c]; hi[c] = any ? std::max(hi[c], b[3 + c]) : b[3 + c]; }
        any = true;
    }
}

// ---- one pass ---------------------------------------------------------------------------------------
// What the stages of a pass share.  Device pointers live in the context arena until the pass returns.
struct RegPass {
    const RegCall* call;
    RegPassOpts opt;
    hipStream_t s;
    int J, N, Ns;                          // jobs, points of all job clouds, points of the source sides
    bool colored;
    double max_dist_icp;
    std::vector<JobDesc> jobs;
    std::vector<int> job_off;              // [2J + 1]: segments [0, J) = sources, [J, 2J) = targets
    MatchPlan plan;                        // host-side plans of the feature stage; they must outlive their H2D copies (synchronised in RANSAC)
    const float4 *det, *mem;               // the pools
    JobDesc* d_jobs; int* d_job_off; int* d_piece_off; double* d_means;
    float4 *P, *normals, *grad;            // centred job clouds and their features (grad: coloured only)
    BatchGrid gC;                          // cell = ICP correspondence distance
    int2* corr; int* n_corr;               // matching -> RANSAC
    RansacState* rs;                       // null: no RANSAC (point-to-point ICP from the identity)
    IcpState* is;
    void *tok_match, *tok_ransac, *tok_icp;       // stage brackets of the in-process timer (bench.py)
    int timing;                            // diag.timing: 1 = a "[reg]" line per phase
    double t_prev;
    void phase(const char* what);
    void dbg(const char* what) const;      // timing 2: synchronise after every launch group of the search phase
};

int ibl_reg_match_stage(ibl_reg_ctx* ctx, RegPass& ps);        // features of the job clouds, matching -> corr, n_corr
int ibl_reg_ransac_stage(ibl_reg_ctx* ctx, RegPass& ps);       // corr -> rs
int ibl_reg_icp_stage(ibl_reg_ctx* ctx, RegPass& ps);          // rs (or identity) -> is
