// engine/layout.h — what every part of engine.hip shares: the error path (set_error, HIP_TRY), the sizes and status
// bits, KernelId, the structs the kernels take by value (TreeCtl, LeafRec, HostLeaf, Pool, Trees) and the 16-byte
// node record's pack / unpack helpers. A part of engine.hip's one translation unit, like its siblings in engine/:
// each includes the siblings whose names it uses, and is guarded by #pragma once as the other csrc/ headers are.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "uttt_bits.h"
#include "uttt_engine.h"

namespace uttt {

// ------------------------------------------------------------------ errors --
void set_error(const char *fmt, ...);  // rules_api.cpp (uttt_last_error)

#define HIP_TRY(expr)                                                                        \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess) {                                                              \
            set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            return UTTT_ERR_HIP;                                                             \
        }                                                                                    \
    } while (0)

// ------------------------------------------------------------------ layout --
constexpr int kWave = 64;
constexpr int kWavesPerBlock = 4;
constexpr int kBlock = kWave * kWavesPerBlock;
constexpr int kMaxDepth = 128;  // path slots: lane d holds path[d] and path[64 + d]
constexpr int kMaxPlies = 81;   // a game fills at most every cell
constexpr int kNone = 0x7fffffff;

constexpr int32_t kLive = 1;
constexpr int32_t kErrCapacity = 2;
constexpr int32_t kErrDepth = 4;
constexpr int32_t kErrSelect = 8;
constexpr int32_t kErrNonFinite = 16;  // the evaluator returned a NaN / Inf legal prior or value
constexpr int32_t kErrMask = kErrCapacity | kErrDepth | kErrSelect | kErrNonFinite;

// a failed tree's status -> message and UTTT_ERR_* (the checks that raise it are at the move / search end)
static const char *tree_error_text(uint32_t st) {
    return (st & kErrCapacity)    ? "node pool exhausted"
           : (st & kErrDepth)     ? "path deeper than 128"
           : (st & kErrNonFinite) ? "non-finite evaluator output (NaN or Inf in a legal prior or the value)"
                                  : "no selectable child (NaN statistics)";
}
static int tree_error_code(uint32_t st) {
    return (st & kErrCapacity) || (st & kErrDepth) ? UTTT_ERR_CAPACITY
           : (st & kErrNonFinite)                  ? UTTT_ERR_NONFINITE
                                                   : UTTT_ERR_ARG;
}

enum KernelId {
    kKSelect = 0, kKApply, kKEncode, kKScan, kKMoveEnd, kKHash,
    // select latency telemetry (counters only, no launches): dependent tree levels walked
    // (sum over trees of sum over descents of depth + 1), trees that descended, the current
    // launch's slowest tree (folded into the sum by k_scan after every select), that sum
    kKSelLevels, kKSelTrees, kKSelMax, kKSelMaxSum,
    // dependent memory round trips (the latency model's unit): sum over trees, the current launch's
    // slowest tree, that slowest count summed over launches
    kKSelTrips, kKSelTripMax, kKSelTripMaxSum,
    // the slowest-tree rows of odd rounds in uttt_rounds_hash_move's per-block form (k_round1 with part_host):
    // each round folds the previous round's rows at its start, so no round needs a last block
    kKSelMaxB, kKSelTripMaxB,
    kKPlayout,  // k_playout_leaves / k_playout_states launches
    kKSolve,    // k_solve_states launches
    kKSolveLeaves,  // k_solve_leaves launches
    kKSymLeaves,    // k_sym_leaves launches
    kKSymRows,      // k_sym_rows launches
    kKRootNoise,    // k_root_noise launches
    kKReroot,       // k_reroot launches
    kKernelCount
};
static_assert(kKSolveLeaves == 17 && kKSymRows == 19 && kKRootNoise == 20 && kKReroot == 21, "the public header and _lib.KERNELS state the ids");

// Device counters are striped: counter i of a row lives in kStripes 128-byte slots, and a workgroup
// adds into slot (blockIdx & (kStripes - 1)), so thousands of waves finishing together do not
// serialize on one address (the host sums the slots).
constexpr int kStripes = 32;
constexpr int kStripeStride = 16;  // u64 per slot: 128 B
constexpr int kRow = kStripes * kStripeStride;  // u64 per counter
__device__ __forceinline__ unsigned long long *stripe_of(unsigned long long *row) {
    return row + (size_t)(blockIdx.x & (kStripes - 1)) * kStripeStride;
}

struct TreeCtl {
    int32_t sims_done;
    int32_t node_count;
    int32_t status;
    int32_t pad;
};

struct LeafRec {
    int32_t node;
    int32_t depth;
    int32_t k;
    int32_t pad;
};

// A single-tree search's round result in fine-grained pinned host memory (round 5, uttt_search_select_host):
// k_scan stores the counts, the pending leaf's state and its copies, then the tag (a system-scope release),
// and the host polls the tag: one select per flush costs no copy operation and no stream synchronisation
// (the reference's flush loop, uttt_mcts.cpp:109-167, runs in-process).
struct HostLeaf {
    int32_t count, stopped, left, tag;
    int32_t k, pad0, pad1, pad2;
    uttt_state_t state;
};

// One node (round 4: four SoA arrays N, W, P, LINK became one record, so the PUCT scan loads a child
// with one dwordx4 and an expansion stores a child with one):
//   .x W (f32 bits)   .y P (f32 bits)
//   .z meta: visits N (bits 0-15) | action (16-22) | L = |legal| of the node's state, the size of
//      each of its child blocks (23-29) | kMetaP64 (30) | kMetaWF32 (31)
//   .w link: first child (bits 0-19) | k = its child blocks (20-31)
// Limits: max_sims <= 4095 (k and N fit; the pool cap 82 + 81 * max_sims < 2^20 first-child indices).
struct Pool {
    uint4 *rec;
    int64_t cap;
};
constexpr int kMaxSimsRec = UTTT_MAX_SIMS;
static_assert(82 + 81ll * kMaxSimsRec < (1ll << 20), "first-child index: 20 bits");
constexpr int kCountRing = 8;  // host-visible count slots per engine (uttt_search_select_async_tag, uttt_round_hash_async)

struct Trees {
    TreeCtl *ctl;
    uttt_state_t *root;
    uttt_state_t *leaf;
    LeafRec *rec;
    int32_t *path;    // [tree][kMaxDepth]
    uint4 *path_rec;  // [tree][kMaxDepth]: the path nodes' records as the select read them (k_apply's back-up
                      // starts from them instead of re-reading each node: one dependent round trip less)
    int32_t *pending; // [tree]: 0 nothing, 2 stopped by the select budget, 1 / 3 a queued leaf (3: the
                      // tree has simulations left after it) | the leaf's depth << 8
    int32_t *tree_of; // [slot]
    int32_t *depth_of; // [slot]: the queued leaf's depth (k_apply loads only the path entries it uses)
    int32_t *count;   // [0] pending leaves this round, [1] trees stopped by the select budget,
                      // [2] trees with simulations left after this round's apply
    int32_t n_trees;
    int32_t sims;
    int32_t batch;
    int32_t py;  // 1: pv_mcts.py semantics (arena), 0: cpp/uttt_mcts.cpp (self-play)
    int32_t budget;  // in-place completions per tree and select launch (kSelectBudget; UTTT_SELECT_BUDGET)
};
// count[3]: nonzero once any tree of the search has failed (reset by k_begin): the asynchronous move end reads
// it instead of a launch that scans every tree's status (k_finalize finds the first failed tree only then)
__device__ __forceinline__ void flag_tree_error(const Trees &tr) { atomicOr(tr.count + 3, 1); }

// record packing (Pool)
constexpr uint32_t kNoAction = 0x7Fu;
__host__ __device__ __forceinline__ uint32_t make_meta(uint32_t action, uint32_t L) {  // N = 0
    return ((action & 0x7Fu) << 16) | ((L & 0x7Fu) << 23);
}
__host__ __device__ __forceinline__ int meta_n(uint32_t m) { return (int)(m & 0xFFFFu); }
__host__ __device__ __forceinline__ int meta_action(uint32_t m) { return (int)((m >> 16) & 0x7Fu); }
__host__ __device__ __forceinline__ int meta_L(uint32_t m) { return (int)((m >> 23) & 0x7Fu); }
// py semantics only (pv_mcts.py, NumPy 2 scalar promotion):
constexpr uint32_t kMetaP64 = 1u << 30;   // this node's children carry float64 uniform priors
constexpr uint32_t kMetaWF32 = 1u << 31;  // this node's w has become np.float32 (a network value)
constexpr uint32_t kMetaLMask = 0x7Fu << 23;
__host__ __device__ __forceinline__ uint32_t make_link(uint32_t first, uint32_t k) { return (first & 0xFFFFFu) | (k << 20); }
__host__ __device__ __forceinline__ int link_first(uint32_t l) { return (int)(l & 0xFFFFFu); }
__host__ __device__ __forceinline__ int link_k(uint32_t l) { return (int)(l >> 20); }
__device__ __forceinline__ uint4 new_child(float p, uint32_t action) {
    return make_uint4(0u, __float_as_uint(p), make_meta(action, 0u), 0u);
}

}  // namespace uttt
