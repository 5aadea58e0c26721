// engine.hip — batched PV-MCTS + self-play for MI355X (gfx950, wave64).
//
// Many independent PUCT trees live in flat pools in HBM, one 16-byte record per
// node: {W f32 value sum, P f32 prior, meta (visits N : 16 | action : 7 | |legal| : 7
// | 2 flags), link (first child : 20 | k copies : 12)}, indexed t * cap + local, the
// root at local 0. A node's children are one contiguous block of k*|legal| records
// (k = copies of the flushed leaf, uttt_mcts.cpp:121-135 + :38-43 append semantics),
// so the PUCT scan reads one 16-byte record per child, fully coalesced. States are never stored per node: a descent replays
// the actions from the root on bitboards (uttt_bits.h).
//
// One round (uttt_mcts.cpp:109-167, all trees in lock-step):
//   k_select  one wave per tree: descend by PUCT (wave arg-max, first index
//             wins ties), back up terminal simulations in place, stop at the
//             first unexpanded leaf -> pending record (node, path, k).
//   k_scan    one block: pending flags -> dense slots in tree order.
//   k_encode  one thread per input element: leaf -> NCHW (3,9,9) f32 row.
//   (evaluator: DualNetwork under PyTorch-ROCm, or k_hash_eval)
//   k_apply   one wave per pending leaf: legal-mask + sequential f32
//             renormalisation, k child blocks, k back-ups along the path.
// Self-play (self_play_cpp.py) adds k_move_end (scores, f64 policy target,
// numpy-legacy MT19937 choice, records), k_finalize (refill + arena offsets)
// and k_archive.
//
// One translation unit. All device code lives in engine/, included here in this order, which is the order of
// definition in the code object (a header includes only headers above it); the host side follows below:
//   layout.h      errors, HIP_TRY, constants, KernelId, TreeCtl / LeafRec / HostLeaf / Pool / Trees, node records
//   wave.h        lane / wave helpers, DPP arg-max, host-visible stores
//   cache.h       EvalCache: probe, lookup, insert
//   expand.h      legal masks, f32 sums, expand_backup, init_root, k_begin
//   symmetry.h    k_sym_leaves, k_sym_rows: the pending leaves through a symmetry, the rows mapped back
//   select.h      k_select's phase clock, the PUCT group scan, select_wave, k_select
//   scan.h        the block scans, k_scan, k_encode
//   apply.h       stop_tree, apply_wave, k_apply
//   rounds.h      k_flush1, input_words, hash_leaf_row, k_round1, k_apply_tree: the fused rounds
//   evaluators.h  k_hash_eval, k_hash_leaves, the playout and solver kernels; root_scores, k_root_visits / _scores
//   search1.h     Search1Host, k_search1: a one-tree search as one resident wave
//   selfplay.h    Slot / GameEntry / SelfPlay, k_move_end, k_finalize, MT19937 seeding, k_archive, k_hwc
//   noise.h       k_root_noise, k_root_priors: Dirichlet noise mixed into the roots' priors, the priors read back
//   reroot.h      k_reroot: tree reuse, the played move's subtree copied to the front of the tree's other pool
//   match.h       Match, k_match_move, k_match_lists: two players' games on the device, the searched move played
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "engine_mem.h"
#include "uttt_bits.h"
#include "uttt_engine.h"
#include "uttt_noise.h"
#include "uttt_playout.h"
#include "uttt_solve.h"
#include "uttt_sym.h"

#include "engine/layout.h"
#include "engine/wave.h"
#include "engine/cache.h"
#include "engine/expand.h"
#include "engine/symmetry.h"
#include "engine/select.h"
#include "engine/scan.h"
#include "engine/apply.h"
#include "engine/rounds.h"
#include "engine/evaluators.h"
#include "engine/search1.h"
#include "engine/selfplay.h"

// Root noise (k_root_noise, k_root_priors): the last kernels of the translation unit, behind every kernel of the
// round loop and the move end, whose places in the code object they leave as they were
#include "engine/noise.h"
namespace uttt {
static_assert(offsetof(Slot, ply) == offsetof(Slot, game) + offsetof(NoiseKey, ply) && offsetof(NoiseKey, stream) == 0,
              "k_root_noise reads a slot's game and ply as one NoiseKey");
}  // namespace uttt
// Tree reuse (k_reroot): behind the noise kernels, for the same reason
#include "engine/reroot.h"
// Match play (k_match_move, k_match_lists): the last of all, for the same reason
#include "engine/match.h"

// ============================================================== host side ==
using namespace uttt;

// The allocate / free pairs behind the engine's buffers (engine_mem.h). Every block the engine owns is a
// DevBuf or a PinBuf member of uttt_engine: `delete e` frees them all, a failed growth leaves an empty buffer.
struct DevMem {
    static void *alloc(size_t bytes) {
        void *p = nullptr;
        const hipError_t r = hipMalloc(&p, bytes ? bytes : 16);
        if (r != hipSuccess) set_error("hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(r));
        return r == hipSuccess ? p : nullptr;
    }
    static void free(void *p) { (void)hipFree(p); }
};
template <unsigned Flags>
struct PinMem {
    static void *alloc(size_t bytes) {
        void *p = nullptr;
        if (hipHostMalloc(&p, bytes, Flags) == hipSuccess) return p;
        set_error("hipHostMalloc failed");
        return nullptr;
    }
    static void free(void *p) { (void)hipHostFree(p); }
};
template <typename T>
using DevBuf = Buf<T, DevMem>;
template <typename T>
using PinBuf = Buf<T, PinMem<hipHostMallocCoherent>>;  // fine-grained: the device's system-scope stores land at once

struct uttt_engine {
    int device = 0;
    int max_trees = 0;
    int max_sims = 0;
    int64_t cap = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    // what the kernels take by value: raw pointers, filled from the owners below (alloc_n)
    Pool pool{};
    Trees tr{};
    // tree reuse (uttt_engine_set_tree_reuse): the to-space k_reroot copies into, allocated when reuse is first
    // switched on; pool.rec and pool2.rec change places after every k_reroot launch
    Pool pool2{};
    DevBuf<uint4> m_rec2;
    DevBuf<int32_t> d_actions;  // uttt_search_reroot's actions
    bool tree_reuse = false;
    bool reuse_ready = false;   // pool holds the trees of this self-play run's last ended move
    DevBuf<uint4> m_rec, m_path_rec;
    DevBuf<TreeCtl> m_ctl;
    DevBuf<uttt_state_t> m_root, m_leaf;
    DevBuf<LeafRec> m_leafrec;
    DevBuf<int32_t> m_path, m_pending, m_tree_of, m_depth_of, m_count;
    Buf<int32_t, PinMem<hipHostMallocDefault>> h_count;  // pinned
    PinBuf<int32_t> h_ring;   // kCountRing x {pending, stopped, left, tag}, k_scan-written
    PinBuf<HostLeaf> h_leaf;  // a one-tree round's result (uttt_search_select_host)
    PinBuf<float> h_eval;     // its evaluation, read by k_apply (uttt_search_apply_host):
                              // [rows][96] policy, [rows] value, one int32 0 (the per-copy row base)
    int64_t h_eval_rows = 0;
    // a hash round's evaluation staged by uttt_round_hash_async (rows by tree), applied by the next round's
    // k_round1 (or by flush_dev_apply before any other call that reads the trees); UTTT_FUSED_ROUNDS=0: separate
    // launches, nothing staged
    const float *dev_apply_policy = nullptr, *dev_apply_value = nullptr;
    bool dev_apply_staged = false;
    // the resident one-tree search (uttt_search1_*, k_search1): its host block and evaluation rows
    PinBuf<char> s1_mem;          // Search1Host, then policy [cap][96], value [cap]
    Search1Host *h_s1 = nullptr;  // s1_mem's head
    int64_t s1_cap = 0;
    int32_t s1_seq = 0;
    bool s1_alive = false;  // a k_search1 wave may still be resident on the stream
    uttt_state_t s1_root{};
    float s1_temperature = 0.0f;
    DevBuf<uint32_t> d_r1ctl;     // k_round1's arrival counters and per-block partials (zero between rounds)
    // uttt_rounds_hash_move's per-block count words: host [kCountRing][part_cap], device [2][part_cap] (the
    // previous round's, for the empty-round check)
    PinBuf<uint32_t> h_part;
    DevBuf<uint32_t> d_part;
    int32_t part_cap = 0;
    uint32_t round_parity = 0;  // the per-block rounds' select-statistics parity (alternates every round)
    int32_t host_apply_rows = 0;  // a one-tree evaluation staged by uttt_search_apply_host, applied by the next
                                  // k_flush1 (or by flush_host_apply before any other call that reads the tree)
    int32_t leaf_tag = 0;
    DevBuf<int32_t> d_rowbase;  // with the two scratch buffers one group (ensure_scratch)
    DevBuf<float> d_pol_scratch, d_val_scratch;
    int64_t scratch_rows = 0;
    DevBuf<uttt_state_t> d_po_states;  // uttt_playouts: the positions and their [wins | losses], one group
    DevBuf<int32_t> d_po_counts;
    int64_t po_rows = 0;
    DevBuf<uttt_state_t> d_sv_states;  // uttt_solve: the positions, their [value | action | status | 81 action
    DevBuf<int8_t> d_sv_out;           // values] bytes and their node counts, one group
    DevBuf<int64_t> d_sv_nodes;
    int64_t sv_rows = 0;
    DevBuf<float> d_scores;
    DevBuf<int32_t> d_nlegal, d_visits;
    // uttt_engine_device_bytes: what alloc_n allocated plus the engine's own cache table, as before the buffers
    // had owners; the blocks grown on demand (scratch, playouts, arena, game table) and pinned memory are not
    // counted (counting them would change what callers see)
    int64_t bytes = 0;
    // round state
    int phase = 0;  // 0 idle, 1 search begun (select next), 2 selected (apply next),
                    // 3 selected without reading the count (uttt_search_select_async; apply next)
    int n_pending = 0;
    bool selfplay = false;
    // self-play
    SelfPlay sp{};  // raw pointers, filled from these owners; the arena's four grow as one group (sp.arena_cap)
    DevBuf<Slot> m_slot;
    DevBuf<uint32_t> m_mt_key;
    DevBuf<int32_t> m_mt_pos, m_live, m_work;
    DevBuf<uttt_state_t> m_ply_state, m_ar_state;
    DevBuf<double> m_ply_policy, m_ar_policy;
    DevBuf<int8_t> m_ply_action, m_ar_action, m_ar_value;
    DevBuf<GameEntry> m_games;
    DevBuf<int64_t> m_ctr;
    int64_t sp_arena_used = 0;
    PinBuf<int64_t> h_move;             // [0..3] sp.ctr after the last move end, [4] error word
    DevBuf<unsigned long long> d_err;   // first failed tree of a move: (tree << 32) | status, or ~0
    // evaluation cache (off unless uttt_engine_set_cache): `cache` is the view the kernels take; the table
    // is this engine's (m_cache_*) or, after uttt_engine_share_cache, another engine's (nothing owned here)
    EvalCache cache{};
    DevBuf<uint32_t> m_cache_flag;
    DevBuf<char> m_cache_rec;
    int cache_log2 = 0;
    int cache_clear_every = 0;
    bool cache_owner = true;  // false: the table belongs to another engine (uttt_engine_share_cache)
    int64_t moves = 0;
    DevBuf<unsigned long long> d_cache_ctr;
    // root noise (uttt_engine_set_root_noise): off while noise_eps is 0
    float noise_eps = 0.0f, noise_alpha = 1.0f;
    uint64_t noise_seed = 0;
    // telemetry
    bool timing = false;
    DevBuf<unsigned long long> d_bytes;  // [kKernelCount]
    struct Ev {
        int kid;
        hipEvent_t a, b;
    };
    std::vector<Ev> pending_ev;
    std::vector<hipEvent_t> ev_pool;
    double ms[kKernelCount] = {};
    int64_t launches[kKernelCount] = {};
};

namespace {

// n elements in owner b, counted in uttt_engine_device_bytes; view (optional): the kernels' raw pointer to it
template <typename T>
int alloc_n(uttt_engine *e, DevBuf<T> &b, size_t n, T **view = nullptr) {
    if (int rc = b.grow((int64_t)n)) return rc;
    if (view) *view = b;
    e->bytes += (int64_t)(n ? n * sizeof(T) : 16);
    return UTTT_OK;
}

hipEvent_t get_event(uttt_engine *e) {
    if (!e->ev_pool.empty()) {
        hipEvent_t ev = e->ev_pool.back();
        e->ev_pool.pop_back();
        return ev;
    }
    hipEvent_t ev;
    // timing-only events: no system-scope fence when recorded (the default one flushes caches at
    // every record; with ~8 timed launches per round that was visible in the tree-only rounds). No
    // host reads data through these events (the counts and counters are system-scope stores).
    if (hipEventCreateWithFlags(&ev, hipEventDisableSystemFence) != hipSuccess) return nullptr;
    return ev;
}

struct TimedLaunch {
    uttt_engine *e;
    int kid;
    hipEvent_t a = nullptr, b = nullptr;
    TimedLaunch(uttt_engine *e_, int kid_) : e(e_), kid(kid_) {
        e->launches[kid]++;
        if (e->timing) {
            a = get_event(e);
            b = get_event(e);
            if (a) (void)hipEventRecord(a, e->stream);
        }
    }
    ~TimedLaunch() {
        if (e->timing && a && b) {
            (void)hipEventRecord(b, e->stream);
            e->pending_ev.push_back({kid, a, b});
        }
    }
};

// One kernel launch whose time the engine's telemetry keeps (round 5): with timing on, the start and
// stop events are the dispatch's own (hipExtLaunchKernelGGL records them when the kernel starts and
// completes, as rocprofv3's kernel trace measures it), not marker packets around the launch: a marker
// pair added ~10 us per launch to the tree kernels (tree-only k_select 27.9 us under rocprofv3 against
// 38.0 us between markers, k_apply 8.5 against 18.7; gpurun_out/t5a, profiles/r5/summary_tree_only.md).
template <typename K, typename... Args>
void timed_launch(uttt_engine *e, int kid, K kernel, dim3 grid, dim3 block, Args... args) {
    e->launches[kid]++;
    if (e->timing) {
        hipEvent_t a = get_event(e), b = get_event(e);
        if (a && b) {
            hipExtLaunchKernelGGL(kernel, grid, block, 0, e->stream, a, b, 0, args...);
            e->pending_ev.push_back({kid, a, b});
            return;
        }
        if (a) e->ev_pool.push_back(a);
        if (b) e->ev_pool.push_back(b);
    }
    hipLaunchKernelGGL(kernel, grid, block, 0, e->stream, args...);
}

// Fold finished event pairs into the totals (pairs whose end has not been reached yet, e.g.
// behind the asynchronous rounds, stay pending).
void drain_events(uttt_engine *e) {
    size_t keep = 0;
    for (auto &ev : e->pending_ev) {
        if (hipEventQuery(ev.b) == hipErrorNotReady) {
            e->pending_ev[keep++] = ev;
            continue;
        }
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, ev.a, ev.b) == hipSuccess) e->ms[ev.kid] += ms;
        e->ev_pool.push_back(ev.a);
        e->ev_pool.push_back(ev.b);
    }
    e->pending_ev.resize(keep);
}

unsigned long long *stats_ptr(uttt_engine *e) { return e->timing ? e->d_bytes.get() : nullptr; }
unsigned long long *bytes_ptr(uttt_engine *e, int kid) { return e->timing ? e->d_bytes + (size_t)kid * kRow : nullptr; }

int check_launch() {
    hipError_t r = hipGetLastError();
    if (r != hipSuccess) {
        set_error("kernel launch failed: %s", hipGetErrorString(r));
        return UTTT_ERR_HIP;
    }
    return UTTT_OK;
}

int grid_waves(int waves) { return (waves + kWavesPerBlock - 1) / kWavesPerBlock; }

int ensure_scratch(uttt_engine *e, int64_t rows) {
    if (rows <= e->scratch_rows) return UTTT_OK;
    int64_t n = e->scratch_rows ? e->scratch_rows : 1024;
    while (n < rows) n *= 2;
    return grow_group(e->scratch_rows, n, e->d_pol_scratch, n * 81, e->d_val_scratch, n, e->d_rowbase,
                      std::max<int64_t>(n, e->max_trees));
}

// Wait for words the device stores into fine-grained host memory: spin until ready(), no stream sync. The
// failure checks run only for a wait past 20 ms, then every 1,024 polls: a stream query goes through the
// runtime's locks and cost tree-only self-play 7% when made every ~40 us while the rounds ran (round 6). A
// failed stream is an error; on_drained() answers a stream that finished without the words (an error code, or
// UTTT_OK after relaunching what stores them); `what` names the result in the 60 s timeout's message.
template <typename Ready, typename Drained>
int spin_wait(uttt_engine *e, const char *what, Ready &&ready, Drained &&on_drained) {
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned it = 1; !ready(); ++it) {
        if ((it & 1023u) == 0u && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(20)) {
            const hipError_t q = hipStreamQuery(e->stream);
            if (q != hipSuccess && q != hipErrorNotReady) {
                set_error("engine stream failed: %s", hipGetErrorString(q));
                return UTTT_ERR_HIP;
            }
            if (q == hipSuccess && !ready())
                if (int rc = on_drained()) return rc;
            if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(60)) {
                set_error("engine: %s not stored within 60 s", what);
                return UTTT_ERR_HIP;
            }
        }
        __builtin_ia32_pause();
    }
    return UTTT_OK;
}
// on_drained for a wait nothing can restart: the error `text`
auto drained_error(const char *text) {
    return [text] {
        set_error("%s", text);
        return UTTT_ERR_HIP;
    };
}

}  // namespace

namespace uttt {
// For the evaluator kernels (nn_kernels.hip): the pending leaves of the current round.
// After uttt_search_select_async the count is on the device only: *n = -1, *n_dev points at
// it and *max_n bounds it (launch grids sized for max_n, kernels exit past *n_dev).
int engine_pending_view(uttt_engine_t *e, const uttt_state_t **leaf, const int32_t **tree_of, int32_t *n,
                        const int32_t **n_dev, int32_t *max_n, hipStream_t *stream) {
    if (!e) return UTTT_ERR_ARG;
    if (e->phase != 2 && e->phase != 3) {
        set_error("no pending leaves (call uttt_search_select first)");
        return UTTT_ERR_ORDER;
    }
    *leaf = e->tr.leaf;
    *tree_of = e->tr.tree_of;
    *n = e->phase == 2 ? e->n_pending : -1;
    *n_dev = e->phase == 3 ? e->tr.count : nullptr;
    *max_n = e->tr.n_trees;
    *stream = e->stream;
    return UTTT_OK;
}
}  // namespace uttt

extern "C" {

const char *uttt_version(void) { return "uttt-mi355x 0.1 (gfx950)"; }

int uttt_engine_create(int32_t device, int32_t max_trees, int32_t max_sims, uttt_engine_t **out) {
    if (!out || max_trees <= 0 || max_trees >= (1 << 21) || max_sims <= 0 || max_sims > kMaxSimsRec) {
        // (k_scan packs its three per-round counts into 21-bit fields)
        set_error("uttt_engine_create: bad arguments (max_trees=%d of at most 2097151, max_sims=%d of at most %d)",
                  max_trees, max_sims, kMaxSimsRec);
        return UTTT_ERR_ARG;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        set_error("no HIP device visible");
        return UTTT_ERR_NODEVICE;
    }
    if (device < 0 && hipGetDevice(&device) != hipSuccess) device = 0;
    if (device < 0 || device >= ndev) {
        set_error("device %d out of range (%d visible)", device, ndev);
        return UTTT_ERR_NODEVICE;
    }
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        set_error("device %d is %s; this engine is built for gfx950 (MI355X)", device, prop.gcnArchName);
        return UTTT_ERR_NODEVICE;
    }
    HIP_TRY(hipSetDevice(device));
    uttt_engine *e = new uttt_engine();
    e->device = device;
    e->max_trees = max_trees;
    e->max_sims = max_sims;
    e->cap = 82 + 81ll * max_sims;  // root + 81 children + 81 per consumed simulation (exact bound)
    int rc = UTTT_OK;
    auto fail = [&](int code) {
        uttt_engine_destroy(e);
        return code;
    };
    if (hipStreamCreateWithFlags(&e->own_stream, hipStreamNonBlocking) != hipSuccess) return fail(UTTT_ERR_HIP);
    e->stream = e->own_stream;
    const size_t nodes = (size_t)max_trees * (size_t)e->cap;
    e->pool.cap = e->cap;
    if ((rc = alloc_n(e, e->m_rec, nodes, &e->pool.rec))) return fail(rc);
    if ((rc = alloc_n(e, e->m_ctl, max_trees, &e->tr.ctl)) || (rc = alloc_n(e, e->m_root, max_trees, &e->tr.root)) ||
        (rc = alloc_n(e, e->m_leaf, max_trees, &e->tr.leaf)) || (rc = alloc_n(e, e->m_leafrec, max_trees, &e->tr.rec)) ||
        (rc = alloc_n(e, e->m_path, (size_t)max_trees * kMaxDepth, &e->tr.path)) ||
        (rc = alloc_n(e, e->m_path_rec, (size_t)max_trees * kMaxDepth, &e->tr.path_rec)) ||
        (rc = alloc_n(e, e->m_pending, max_trees, &e->tr.pending)) ||
        (rc = alloc_n(e, e->m_tree_of, max_trees, &e->tr.tree_of)) ||
        (rc = alloc_n(e, e->m_depth_of, max_trees, &e->tr.depth_of)) || (rc = alloc_n(e, e->m_count, 4, &e->tr.count)) ||
        (rc = alloc_n(e, e->d_scores, (size_t)max_trees * 81)) || (rc = alloc_n(e, e->d_visits, (size_t)max_trees * 81)) ||
        (rc = alloc_n(e, e->d_nlegal, max_trees)) || (rc = alloc_n(e, e->d_bytes, kKernelCount * kRow)) ||
        (rc = alloc_n(e, e->d_cache_ctr, 4 * kRow)) ||
        (rc = alloc_n(e, e->d_r1ctl, (size_t)kR1Partial + (size_t)grid_waves(max_trees))) ||
        (rc = alloc_n(e, e->d_err, 1)))
        return fail(rc);
    if ((rc = e->h_move.grow(5)) || (rc = e->h_ring.grow(4 * kCountRing)) || (rc = e->h_leaf.grow(1)) ||
        (rc = e->h_count.grow(4)))
        return fail(rc);
    memset(e->h_ring, 0, sizeof(int32_t) * 4 * kCountRing);
    memset(e->h_leaf, 0, sizeof(HostLeaf));
    if (hipMemsetAsync(e->tr.ctl, 0, sizeof(TreeCtl) * max_trees, e->stream) != hipSuccess ||
        hipMemsetAsync(e->d_bytes, 0, sizeof(unsigned long long) * kKernelCount * kRow, e->stream) != hipSuccess ||
        hipMemsetAsync(e->d_cache_ctr, 0, sizeof(unsigned long long) * 4 * kRow, e->stream) != hipSuccess ||
        hipMemsetAsync(e->d_r1ctl, 0, sizeof(uint32_t) * ((size_t)kR1Partial + (size_t)grid_waves(max_trees)),
                       e->stream) != hipSuccess ||
        hipStreamSynchronize(e->stream) != hipSuccess) {
        set_error("engine init memset failed");
        return fail(UTTT_ERR_HIP);
    }
    e->tr.n_trees = 0;
    *out = e;
    return UTTT_OK;
}

static int search1_stop(uttt_engine *e);
int uttt_engine_destroy(uttt_engine_t *e) {
    if (!e) return UTTT_OK;
    (void)hipSetDevice(e->device);
    (void)search1_stop(e);  // a resident one-tree search wave exits first
    if (e->stream) (void)hipStreamSynchronize(e->stream);
    drain_events(e);
    for (hipEvent_t ev : e->ev_pool) (void)hipEventDestroy(ev);
    if (e->own_stream) (void)hipStreamDestroy(e->own_stream);
    delete e;  // every device and pinned block: the members' destructors (engine_mem.h)
    return UTTT_OK;
}

int uttt_engine_own_stream(uttt_engine_t *e, void **stream) {
    if (!e || !stream) return UTTT_ERR_ARG;
    *stream = (void *)e->own_stream;
    return UTTT_OK;
}

int uttt_engine_set_stream(uttt_engine_t *e, void *stream) {
    if (!e) return UTTT_ERR_ARG;
    // NULL is the null (legacy default) stream — what torch.cuda.current_stream()
    // is unless the caller made one; the engine's own stream is non-blocking and
    // would not be ordered against it.
    e->stream = (hipStream_t)stream;
    return UTTT_OK;
}

int64_t uttt_engine_device_bytes(const uttt_engine_t *e) { return e ? e->bytes : 0; }

static int search_begin_common(uttt_engine *e, int32_t n_trees, int32_t sims, int32_t batch) {
    if (int rc0 = search1_stop(e)) return rc0;  // a resident one-tree search left unfinished
    e->dev_apply_staged = false;  // a staged round of a search that was never ended is dropped with it
    e->host_apply_rows = 0;       // (and a staged one-tree evaluation)
    e->reuse_ready = false;       // (and the trees a self-play move would have carried over)
    if (n_trees <= 0 || n_trees > e->max_trees) {
        set_error("n_trees %d out of range 1..%d", n_trees, e->max_trees);
        return UTTT_ERR_ARG;
    }
    if (sims <= 0 || sims > e->max_sims) {
        set_error("evaluate_count %d out of range 1..%d (engine max_sims)", sims, e->max_sims);
        return UTTT_ERR_ARG;
    }
    e->tr.n_trees = n_trees;
    e->tr.sims = sims;
    // uttt_mcts.cpp:127: a flush happens once the queue holds batch_size entries,
    // so batch_size <= 1 flushes every queued leaf alone.
    e->tr.batch = batch < 1 ? 1 : batch;
    // the select budget changes how a move's simulations are spread over launches, never which
    // simulations run or in what order per tree (results are the same for any value >= 1)
    const char *bv = getenv("UTTT_SELECT_BUDGET");
    const int b = bv ? atoi(bv) : 0;
    e->tr.budget = b >= 1 && b <= 4096 ? b : kSelectBudget;
    e->phase = 1;
    e->n_pending = 0;
    return UTTT_OK;
}

// The start of a search with given semantics (fn: the caller's name for the message): the argument check, then
// search_begin_common
static int begin_with_semantics(uttt_engine *e, const char *fn, const uttt_state_t *roots, int32_t n_trees, int32_t sims,
                                int32_t batch, int32_t semantics) {
    if (!e || !roots || (semantics != UTTT_SEMANTICS_CPP && semantics != UTTT_SEMANTICS_PY)) {
        set_error("%s: bad arguments (semantics 0 = cpp, 1 = py)", fn);
        return UTTT_ERR_ARG;
    }
    HIP_TRY(hipSetDevice(e->device));
    if (int rc = search_begin_common(e, n_trees, sims, batch)) return rc;
    e->tr.py = semantics == UTTT_SEMANTICS_PY ? 1 : 0;
    e->selfplay = false;
    return UTTT_OK;
}

// Root noise, when it is on, behind the k_begin that built the roots (keys: the self-play slots' NoiseKey words, or
// nullptr for a plain search)
static void launch_root_noise(uttt_engine *e, const char *keys, int key_stride) {
    if (!(e->noise_eps > 0.0f)) return;
    timed_launch(e, kKRootNoise, k_root_noise, dim3(grid_waves(e->tr.n_trees)), dim3(kBlock), e->pool, e->tr, keys,
                 key_stride, e->noise_eps, e->noise_alpha, e->noise_seed);
}
// What has no root priors to mix noise into when a search begins (fn) refuses an engine with noise on
static int refuse_root_noise(uttt_engine *e, const char *fn, const char *why) {
    if (!e || !(e->noise_eps > 0.0f)) return UTTT_OK;
    set_error("%s: root noise is on (uttt_engine_set_root_noise) and %s", fn, why);
    return UTTT_ERR_ARG;
}

// Tree reuse is defined for the C++ semantics' append-only trees built by k_begin / k_reroot only
static int refuse_tree_reuse(uttt_engine *e, const char *fn, const char *why) {
    if (!e || !e->tree_reuse) return UTTT_OK;
    set_error("%s: tree reuse is on (uttt_engine_set_tree_reuse) and %s", fn, why);
    return UTTT_ERR_ARG;
}

int uttt_search_begin(uttt_engine_t *e, const uttt_state_t *roots, int32_t n_trees, int32_t sims, int32_t batch) {
    return uttt_search_begin_mode(e, roots, n_trees, sims, batch, UTTT_SEMANTICS_CPP);
}

// A plain search's begin for roots in host memory (uttt_search_begin_mode) or on the device (uttt_match_search_begin;
// kind says which): the checks, the copy into the trees' leaf slots, k_begin, and the root noise when it is on
static int search_begin_roots(uttt_engine *e, const char *fn, const uttt_state_t *roots, int32_t n_trees, int32_t sims,
                              int32_t batch, int32_t semantics, hipMemcpyKind kind) {
    if (semantics == UTTT_SEMANTICS_PY)
        if (int rc = refuse_root_noise(e, fn, "a py root takes its priors from its first flush: use UTTT_SEMANTICS_CPP"))
            return rc;
    if (semantics == UTTT_SEMANTICS_PY)
        if (int rc = refuse_tree_reuse(e, fn, "a py tree's expansions replace: use UTTT_SEMANTICS_CPP")) return rc;
    if (int rc = begin_with_semantics(e, fn, roots, n_trees, sims, batch, semantics)) return rc;
    HIP_TRY(hipMemcpyAsync(e->tr.leaf, roots, sizeof(uttt_state_t) * n_trees, kind, e->stream));
    hipLaunchKernelGGL(k_begin, dim3(grid_waves(n_trees)), dim3(kBlock), 0, e->stream, e->pool, e->tr,
                       (const char *)e->tr.leaf, (int)sizeof(uttt_state_t), (const int32_t *)nullptr,
                       (unsigned long long *)nullptr);
    launch_root_noise(e, nullptr, 0);
    return check_launch();
}

int uttt_search_begin_mode(uttt_engine_t *e, const uttt_state_t *roots, int32_t n_trees, int32_t sims, int32_t batch,
                           int32_t semantics) {
    return search_begin_roots(e, "uttt_search_begin_mode", roots, n_trees, sims, batch, semantics, hipMemcpyHostToDevice);
}

static int flush_host_apply(uttt_engine *e);

// One descent of every tree and the scan of its pending leaves (host_count, optional: a count-ring slot the
// scan also stores the counts and then `tag` into)
static int launch_select_scan(uttt_engine *e, int32_t *host_count, int32_t tag) {
    timed_launch(e, kKSelect, e->tr.py ? k_select<true> : k_select<false>, dim3(grid_waves(e->tr.n_trees)),
                 dim3(kBlock), e->pool, e->tr, e->cache, stats_ptr(e));
    if (int rc = check_launch()) return rc;
    timed_launch(e, kKScan, k_scan, dim3(1), dim3(1024), e->tr, stats_ptr(e), host_count, tag);
    return check_launch();
}

int uttt_search_select(uttt_engine_t *e, float *nn_input, int32_t *n_pending) {
    if (!e || !n_pending) return UTTT_ERR_ARG;
    if (e->phase != 1) {
        set_error("uttt_search_select: call uttt_search_begin (or apply the previous round) first");
        return UTTT_ERR_ORDER;
    }
    HIP_TRY(hipSetDevice(e->device));
    if (int rc0 = flush_host_apply(e)) return rc0;
    int rc = 0, n = 0;
    // trees stopped by the select budget resume in the next launch; when no tree has a
    // leaf but some were stopped, select again (every launch completes >= 1 simulation
    // of each stopped tree, so this ends)
    for (;;) {
        if ((rc = launch_select_scan(e, nullptr, 0))) return rc;
        HIP_TRY(hipMemcpyAsync(e->h_count, e->tr.count, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        drain_events(e);
        n = e->h_count[0];
        if (n > 0 || e->h_count[1] == 0) break;
    }
    if (n > 0 && nn_input) {
        const int total = n * 243;
        timed_launch(e, kKEncode, k_encode, dim3((total + 255) / 256), dim3(256), e->tr, nn_input, n);
    }
    if ((rc = check_launch())) return rc;
    e->n_pending = n;
    e->phase = n > 0 ? 2 : 1;
    *n_pending = n;
    return UTTT_OK;
}

static int select_async_impl(uttt_engine_t *e, int32_t *host_count, int32_t tag = 0);
int uttt_search_select_async(uttt_engine_t *e) { return select_async_impl(e, nullptr); }

int uttt_search_select_async_tag(uttt_engine_t *e, int32_t ring_slot, int32_t tag) {
    if (!e || ring_slot < 0 || ring_slot >= kCountRing) {
        set_error("uttt_search_select_async_tag: ring slot must be in 0..%d", kCountRing - 1);
        return UTTT_ERR_ARG;
    }
    return select_async_impl(e, e->h_ring + 4 * ring_slot, tag);
}

int uttt_search_count_ring(uttt_engine_t *e, const int32_t **ring, int32_t *n_slots) {
    if (!e || !ring || !n_slots) return UTTT_ERR_ARG;
    *ring = e->h_ring;
    *n_slots = kCountRing;
    return UTTT_OK;
}

static int select_async_impl(uttt_engine_t *e, int32_t *host_count, int32_t tag) {
    if (!e) return UTTT_ERR_ARG;
    if (e->phase != 1) {
        set_error("uttt_search_select_async: call uttt_search_begin (or apply the previous round) first");
        return UTTT_ERR_ORDER;
    }
    HIP_TRY(hipSetDevice(e->device));
    if (int rc0 = flush_host_apply(e)) return rc0;
    if (int rc = launch_select_scan(e, host_count, tag)) return rc;
    e->n_pending = -1;
    e->phase = 3;
    return UTTT_OK;
}

int uttt_search_count_copy(uttt_engine_t *e, int32_t *dst) {
    if (!e || !dst) return UTTT_ERR_ARG;
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipMemcpyAsync(dst, e->tr.count, 3 * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    return UTTT_OK;
}

int uttt_search_count_ptr(uttt_engine_t *e, const int32_t **count) {
    if (!e || !count) return UTTT_ERR_ARG;
    *count = e->tr.count;
    return UTTT_OK;
}

int uttt_search_pending(uttt_engine_t *e, uttt_state_t *states, int32_t *copies) {
    if (!e) return UTTT_ERR_ARG;
    if (e->phase != 2) {
        set_error("uttt_search_pending: no pending leaves (call uttt_search_select)");
        return UTTT_ERR_ORDER;
    }
    HIP_TRY(hipSetDevice(e->device));
    const int n = e->n_pending;
    std::vector<int32_t> tree_of(n);
    HIP_TRY(hipMemcpyAsync(tree_of.data(), e->tr.tree_of, sizeof(int32_t) * n, hipMemcpyDeviceToHost, e->stream));
    std::vector<uttt_state_t> leaf(e->tr.n_trees);
    std::vector<LeafRec> rec(e->tr.n_trees);
    HIP_TRY(hipMemcpyAsync(leaf.data(), e->tr.leaf, sizeof(uttt_state_t) * e->tr.n_trees, hipMemcpyDeviceToHost,
                           e->stream));
    HIP_TRY(hipMemcpyAsync(rec.data(), e->tr.rec, sizeof(LeafRec) * e->tr.n_trees, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    for (int i = 0; i < n; ++i) {
        if (states) states[i] = leaf[tree_of[i]];
        if (copies) copies[i] = rec[tree_of[i]].k;
    }
    return UTTT_OK;
}

// Evaluation rows into a pinned block a kernel reads (policy rows at a 96-float stride, 81 used), complete
// before whatever the caller does next to make the device read them (x86 keeps the stores in order; the fence
// keeps the compiler's)
static void stage_rows(float *dst_policy, float *dst_value, const float *policy, int64_t pld, const float *value,
                       int32_t rows) {
    for (int32_t r = 0; r < rows; ++r) {
        memcpy(dst_policy + (size_t)r * 96, policy + (size_t)r * pld, 81 * sizeof(float));
        dst_value[r] = value[r];
    }
    __atomic_thread_fence(__ATOMIC_SEQ_CST);
}

// The staged evaluation's k_apply arguments (pinned host memory; rows 1: one row for the leaf's k copies,
// rows k: one per copy, applied in order, the evaluation cache bypassed as in uttt_search_apply).
struct HostApplyArgs {
    const float *policy, *value;
    const int32_t *rowbase;
    int per_copy;
    EvalCache cache;
};
static HostApplyArgs host_apply_args(uttt_engine *e) {
    HostApplyArgs a;
    a.policy = e->h_eval;
    a.value = e->h_eval + e->h_eval_rows * 96;
    a.rowbase = reinterpret_cast<const int32_t *>(e->h_eval + e->h_eval_rows * 97);
    a.per_copy = e->host_apply_rows > 1 ? 1 : 0;
    a.cache = a.per_copy ? EvalCache{} : e->cache;
    return a;
}

// A round's evaluation staged by uttt_round_hash_async (rows by tree) that no k_round1 has applied yet, applied
// now (by every call that reads, selects in or restarts the trees, uttt_search_select_host included)
static int flush_dev_apply(uttt_engine *e) {
    if (!e->dev_apply_staged) return UTTT_OK;
    e->dev_apply_staged = false;
    timed_launch(e, kKApply, k_apply_tree, dim3(grid_waves(e->tr.n_trees)), dim3(kBlock), e->pool, e->tr, e->cache,
                 e->dev_apply_policy, e->dev_apply_value, bytes_ptr(e, kKApply));
    return check_launch();
}

static int flush_host_apply(uttt_engine *e) {
    if (int rc = flush_dev_apply(e)) return rc;
    if (!e->host_apply_rows) return UTTT_OK;
    const HostApplyArgs a = host_apply_args(e);
    e->host_apply_rows = 0;
    timed_launch(e, kKApply, k_apply, dim3(grid_waves(1)), dim3(kBlock), e->pool, e->tr, a.cache, a.policy,
                 (int64_t)96, a.value, (int64_t)1, a.rowbase, a.per_copy, bytes_ptr(e, kKApply));
    return check_launch();
}

// ---- the resident one-tree search (k_search1) ----
static float *s1_policy(uttt_engine *e) { return reinterpret_cast<float *>(e->h_s1 + 1); }
static float *s1_value(uttt_engine *e) { return s1_policy(e) + (size_t)e->s1_cap * 96; }

// a resident wave left by an unfinished search exits (its exit word) before anything else runs on the stream
static int search1_stop(uttt_engine *e) {
    if (!e->s1_alive) return UTTT_OK;
    __atomic_store_n(&e->h_s1->cmd_exit, 1, __ATOMIC_SEQ_CST);
    e->s1_alive = false;
    HIP_TRY(hipStreamSynchronize(e->stream));
    return UTTT_OK;
}

static int search1_launch(uttt_engine *e, int32_t resume) {
    hipLaunchKernelGGL(e->tr.py ? k_search1<true> : k_search1<false>, dim3(1), dim3(kWave), 0, e->stream, e->pool, e->tr,
                       e->cache, e->s1_root, e->s1_temperature, e->h_s1, (const float *)s1_policy(e),
                       (const float *)s1_value(e), e->s1_seq, resume);
    e->s1_alive = true;
    return check_launch();
}

int uttt_search1_begin(uttt_engine_t *e, const uttt_state_t *root, int32_t sims, int32_t batch, int32_t semantics,
                       float temperature) {
    if (int rc = refuse_root_noise(e, "uttt_search1_begin",
                                   "the resident one-tree search builds its root itself: use uttt_search_begin"))
        return rc;
    if (int rc = refuse_tree_reuse(e, "uttt_search1_begin",
                                   "the resident one-tree search keeps its tree in its own wave: use uttt_search_begin"))
        return rc;
    // (search_begin_common: a resident wave left by an unfinished search exits first)
    if (int rc = begin_with_semantics(e, "uttt_search1_begin", root, 1, sims, batch, semantics)) return rc;
    const int32_t need = e->tr.batch > 16 ? e->tr.batch : 16;  // rows per flush: 1 or k <= batch
    if (need > e->s1_cap) {  // no wave is resident
        const int64_t bytes = (int64_t)(sizeof(Search1Host) + (size_t)need * 97 * sizeof(float) + 16);
        e->h_s1 = nullptr;
        if (int rc = grow_group(e->s1_cap, need, e->s1_mem, bytes)) return rc;
        memset(e->s1_mem, 0, (size_t)bytes);
        e->h_s1 = reinterpret_cast<Search1Host *>(e->s1_mem.get());
    }
    Search1Host *h = e->h_s1;
    h->tag = 0;
    h->gone = 0;
    h->cmd = 0;
    h->cmd_exit = 0;
    h->count = 0;
    __atomic_thread_fence(__ATOMIC_SEQ_CST);
    e->s1_root = *root;
    e->s1_temperature = temperature;
    e->s1_seq = 0;
    e->phase = 1;
    e->n_pending = 0;
    return search1_launch(e, 0);
}

int uttt_search1_next(uttt_engine_t *e, uttt_state_t *leaf, int32_t *copies, int32_t *n_pending) {
    if (!e || !leaf || !copies || !n_pending) return UTTT_ERR_ARG;
    if (e->phase != 1 || !e->h_s1 || !e->s1_alive) {
        set_error("uttt_search1_next: call uttt_search1_begin (or apply the previous leaf) first");
        return UTTT_ERR_ORDER;
    }
    const int32_t want = e->s1_seq + 1;
    Search1Host *h = e->h_s1;
    const int rc = spin_wait(
        e, "one-tree search result", [&] { return __atomic_load_n(&h->tag, __ATOMIC_ACQUIRE) == want; },
        [&]() -> int {
            // the wave timed out waiting for the previous command (the host took over 100 ms): resume it,
            // the command it did not see applied first
            if (__atomic_load_n(&h->gone, __ATOMIC_ACQUIRE) != e->s1_seq || e->s1_seq == 0) {
                set_error("engine: the resident search left without storing its result");
                return UTTT_ERR_HIP;
            }
            h->gone = 0;
            __atomic_thread_fence(__ATOMIC_SEQ_CST);
            return search1_launch(e, 1);
        });
    if (rc) return rc;
    e->s1_seq = want;
    const int n = __atomic_load_n(&h->count, __ATOMIC_ACQUIRE);
    if (n > 0) {
        memcpy(leaf, const_cast<const uttt_state_t *>(&h->leaf), sizeof(uttt_state_t));
        *copies = h->k;
        e->n_pending = 1;
        e->phase = 2;
    } else {
        e->s1_alive = false;  // the wave ends after the search's end
        e->n_pending = 0;
        e->phase = 1;
        const uint32_t st = (uint32_t)__atomic_load_n(&h->status, __ATOMIC_ACQUIRE);
        if (st & kErrMask) {
            set_error("tree 0 failed (status 0x%x: %s)", st, tree_error_text(st));
            return tree_error_code(st);
        }
    }
    *n_pending = n;
    return UTTT_OK;
}

int uttt_search1_apply(uttt_engine_t *e, const float *policy, int64_t pld, const float *value, int32_t rows) {
    if (!e || !policy || !value || pld < 81 || rows < 1) {
        set_error("uttt_search1_apply: bad arguments (policy stride must be >= 81, rows >= 1)");
        return UTTT_ERR_ARG;
    }
    if (e->phase != 2 || !e->s1_alive) {
        set_error("uttt_search1_apply: no pending leaf (call uttt_search1_next)");
        return UTTT_ERR_ORDER;
    }
    Search1Host *h = e->h_s1;
    const int32_t k = h->k;
    if ((rows != 1 && rows != k) || rows > e->s1_cap) {
        set_error("uttt_search1_apply: %d results for a leaf queued %d times (pass 1 or %d)", rows, k, k);
        return UTTT_ERR_ARG;
    }
    // the rows before the command the wave polls (stage_rows' fence)
    stage_rows(s1_policy(e), s1_value(e), policy, pld, value, rows);
    __atomic_store_n(&h->cmd, (uint64_t)(uint32_t)rows << 32 | (uint32_t)e->s1_seq, __ATOMIC_RELEASE);
    e->phase = 1;
    e->n_pending = 0;
    return UTTT_OK;
}

int uttt_search1_scores(uttt_engine_t *e, float *scores, int32_t *n_legal) {
    if (!e || !scores || !n_legal) return UTTT_ERR_ARG;
    if (!e->h_s1 || e->s1_alive || e->phase != 1) {
        set_error("uttt_search1_scores: the search has not ended (uttt_search1_next returns no leaf at its end)");
        return UTTT_ERR_ORDER;
    }
    const Search1Host *h = e->h_s1;
    const int L = h->n_legal;
    for (int i = 0; i < 81; ++i) scores[i] = i < L ? h->scores[i] : 0.0f;
    *n_legal = L;
    return UTTT_OK;
}

int uttt_search1_time_split(uttt_engine_t *e, int32_t *ticks3) {
    if (!e || !ticks3 || !e->h_s1) return UTTT_ERR_ARG;
    const Search1Host *h = e->h_s1;
    ticks3[0] = __atomic_load_n(&h->t_select, __ATOMIC_ACQUIRE);
    ticks3[1] = __atomic_load_n(&h->t_apply, __ATOMIC_ACQUIRE);
    ticks3[2] = __atomic_load_n(&h->t_wait, __ATOMIC_ACQUIRE);
    return UTTT_OK;
}

int uttt_search_select_host(uttt_engine_t *e, uttt_state_t *leaf, int32_t *copies, int32_t *n_pending) {
    if (!e || !leaf || !copies || !n_pending) return UTTT_ERR_ARG;
    if (e->tr.n_trees != 1) {
        set_error("uttt_search_select_host: one-tree searches only (uttt_search_begin with n_trees = 1)");
        return UTTT_ERR_ARG;
    }
    if (e->phase != 1) {
        set_error("uttt_search_select_host: call uttt_search_begin (or apply the previous round) first");
        return UTTT_ERR_ORDER;
    }
    HIP_TRY(hipSetDevice(e->device));
    // a round staged by uttt_round_hash_async on this one-tree search is applied first (k_flush1 applies only
    // host-staged evaluations)
    if (int rc0 = flush_dev_apply(e)) return rc0;
    int rc = 0, n = 0;
    for (;;) {  // the select budget may stop the tree before it queues a leaf: select again (as uttt_search_select)
        const int32_t tag = ++e->leaf_tag;
        const int do_apply = e->host_apply_rows ? 1 : 0;
        HostApplyArgs a = host_apply_args(e);
        e->host_apply_rows = 0;
        e->launches[kKApply] += do_apply;
        timed_launch(e, kKSelect, e->tr.py ? k_flush1<true> : k_flush1<false>, dim3(1), dim3(kWave), e->pool, e->tr,
                     e->cache, a.cache, a.policy, (int64_t)96, a.value, (int64_t)1, a.rowbase, a.per_copy, do_apply,
                     stats_ptr(e), e->h_leaf.get(), tag);
        if ((rc = check_launch())) return rc;
        // (spin, no stream sync; the gated stream queries only take runtime calls off this path)
        if ((rc = spin_wait(e, "round result", [&] { return __atomic_load_n(&e->h_leaf->tag, __ATOMIC_ACQUIRE) == tag; },
                            drained_error("engine: the stream drained without storing the round's tag"))))
            return rc;
        n = __atomic_load_n(&e->h_leaf->count, __ATOMIC_ACQUIRE);
        if (e->timing) drain_events(e);
        if (n > 0 || __atomic_load_n(&e->h_leaf->stopped, __ATOMIC_ACQUIRE) == 0) break;
    }
    if (n > 0) {
        memcpy(leaf, const_cast<const uttt_state_t *>(&e->h_leaf->state), sizeof(uttt_state_t));
        *copies = e->h_leaf->k;
    }
    *n_pending = n;
    e->n_pending = n;
    e->phase = n > 0 ? 2 : 1;
    return UTTT_OK;
}

int uttt_search_apply_host(uttt_engine_t *e, const float *policy, int64_t pld, const float *value, int32_t rows) {
    if (!e || !policy || !value || pld < 81 || rows < 1) {
        set_error("uttt_search_apply_host: bad arguments (policy stride must be >= 81, rows >= 1)");
        return UTTT_ERR_ARG;
    }
    if (e->phase != 2 || e->n_pending != 1 || e->tr.n_trees != 1) {
        set_error("uttt_search_apply_host: no pending leaf of a one-tree search (call uttt_search_select_host)");
        return UTTT_ERR_ORDER;
    }
    const int32_t k = e->h_leaf->k;
    if (rows != 1 && rows != k) {
        set_error("uttt_search_apply_host: %d results for a leaf queued %d times (pass 1 or %d)", rows, k, k);
        return UTTT_ERR_ARG;
    }
    HIP_TRY(hipSetDevice(e->device));
    if (rows > e->h_eval_rows) {
        // grown between rounds only: the k_flush1 that last read the buffer completed before it stored the
        // tag the host has seen
        int64_t cap = e->h_eval_rows ? e->h_eval_rows : 16;
        while (cap < rows) cap *= 2;
        if (int rc = grow_group(e->h_eval_rows, cap, e->h_eval, cap * 97 + 4)) return rc;
        reinterpret_cast<int32_t *>(e->h_eval + cap * 97)[0] = 0;  // the per-copy row base of slot 0
    }
    // the rows before the launch that reads them
    stage_rows(e->h_eval, e->h_eval + e->h_eval_rows * 96, policy, pld, value, rows);
    e->host_apply_rows = rows;  // applied by the next k_flush1 (or flush_host_apply)
    e->phase = 1;
    e->n_pending = 0;
    return UTTT_OK;
}

int uttt_search_apply(uttt_engine_t *e, const float *policy, int64_t pld, const float *value, int64_t vld,
                      int32_t per_copy, int32_t on_device) {
    if (!e || !policy || !value || pld < 81 || vld < 1) {
        set_error("uttt_search_apply: bad arguments (policy stride must be >= 81)");
        return UTTT_ERR_ARG;
    }
    if (e->phase != 2 && e->phase != 3) {
        set_error("uttt_search_apply: no pending leaves (call uttt_search_select)");
        return UTTT_ERR_ORDER;
    }
    if (e->phase == 3 && (per_copy || !on_device)) {
        set_error("uttt_search_apply: after uttt_search_select_async the results must be on the device, one per leaf");
        return UTTT_ERR_ORDER;
    }
    if (per_copy && e->tr.py) {
        set_error("uttt_search_apply: per_copy is the cpp call pattern; py semantics take one result per leaf");
        return UTTT_ERR_ARG;
    }
    HIP_TRY(hipSetDevice(e->device));
    // phase 3: the count is on the device; k_apply reads it (tr.count[0]) and the grid covers every tree
    const int n = e->phase == 3 ? e->tr.n_trees : e->n_pending;
    const int32_t *rowbase = nullptr;
    int64_t rows = n;
    if (per_copy) {
        // rows are grouped per slot: slot i's k_i copies start at sum_{j<i} k_j
        std::vector<int32_t> k(n);
        int rc = uttt_search_pending(e, nullptr, k.data());
        if (rc) return rc;
        std::vector<int32_t> rb(n);
        int64_t acc = 0;
        for (int i = 0; i < n; ++i) {
            rb[i] = (int32_t)acc;
            acc += k[i];
        }
        rows = acc;
        if ((rc = ensure_scratch(e, rows))) return rc;
        HIP_TRY(hipMemcpyAsync(e->d_rowbase, rb.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice, e->stream));
        rowbase = e->d_rowbase;
    }
    const float *dp = policy, *dv = value;
    int64_t dpld = pld, dvld = vld;
    if (!on_device) {
        int rc = ensure_scratch(e, rows);
        if (rc) return rc;
        HIP_TRY(hipMemcpy2DAsync(e->d_pol_scratch, 81 * sizeof(float), policy, (size_t)pld * sizeof(float),
                                 81 * sizeof(float), (size_t)rows, hipMemcpyHostToDevice, e->stream));
        HIP_TRY(hipMemcpy2DAsync(e->d_val_scratch, sizeof(float), value, (size_t)vld * sizeof(float), sizeof(float),
                                 (size_t)rows, hipMemcpyHostToDevice, e->stream));
        dp = e->d_pol_scratch;
        dv = e->d_val_scratch;
        dpld = 81;
        dvld = 1;
    }
    {
        EvalCache c = per_copy ? EvalCache{} : e->cache;  // the reference call pattern bypasses the cache
        timed_launch(e, kKApply, k_apply, dim3(grid_waves(n)), dim3(kBlock), e->pool, e->tr, c, dp, dpld, dv, dvld,
                     rowbase, per_copy ? 1 : 0, bytes_ptr(e, kKApply));
    }
    int rc = check_launch();
    if (rc) return rc;
    if (!on_device) HIP_TRY(hipStreamSynchronize(e->stream));  // host buffers may be freed on return
    e->phase = 1;
    e->n_pending = 0;
    return UTTT_OK;
}

int uttt_eval_hash(uttt_engine_t *e, const float *nn_input, int32_t n, float *policy, float *value) {
    if (!e || !nn_input || !policy || !value || n < 0) return UTTT_ERR_ARG;
    if (n == 0) return UTTT_OK;
    HIP_TRY(hipSetDevice(e->device));
    timed_launch(e, kKHash, k_hash_eval, dim3(grid_waves(n)), dim3(kBlock), nn_input, n, policy, value);
    return check_launch();
}

int uttt_eval_hash_dev(uttt_engine_t *e, float *policy, float *value) {
    if (!e || !policy || !value) return UTTT_ERR_ARG;
    HIP_TRY(hipSetDevice(e->device));
    timed_launch(e, kKHash, k_hash_leaves, dim3(grid_waves(e->tr.n_trees)), dim3(kBlock), e->tr, policy, value);
    return check_launch();
}

static int check_playouts(int32_t playouts) {
    if (playouts < 1 || playouts > kMaxPlayouts) {
        set_error("playouts must be 1..%d (got %d)", kMaxPlayouts, playouts);
        return UTTT_ERR_ARG;
    }
    return UTTT_OK;
}

int uttt_eval_playout_dev(uttt_engine_t *e, int32_t playouts, uint64_t seed, float *policy, float *value) {
    if (!e || !policy || !value) return UTTT_ERR_ARG;
    if (int rc = check_playouts(playouts)) return rc;
    HIP_TRY(hipSetDevice(e->device));
    timed_launch(e, kKPlayout, k_playout_leaves, dim3(grid_waves(e->tr.n_trees)), dim3(kBlock), e->tr, (int)playouts,
                 seed, policy, value);
    return check_launch();
}

int uttt_playouts(uttt_engine_t *e, const uttt_state_t *states, int32_t n, int32_t playouts, uint64_t seed,
                  int32_t *wins, int32_t *losses) {
    if (!e || n < 0 || ((!states || !wins || !losses) && n > 0)) {
        set_error("uttt_playouts: null pointer or negative count");
        return UTTT_ERR_ARG;
    }
    if (int rc = check_playouts(playouts)) return rc;
    for (int32_t i = 0; i < n; ++i) {
        if (states[i].active < -1 || states[i].active > 8) {
            set_error("active_board must be -1..8 (state %d has %d)", i, states[i].active);
            return UTTT_ERR_ARG;
        }
    }
    if (n == 0) return UTTT_OK;
    HIP_TRY(hipSetDevice(e->device));
    if (n > e->po_rows) {
        int64_t rows = e->po_rows ? e->po_rows : 1024;
        while (rows < n) rows *= 2;
        if (int rc = grow_group(e->po_rows, rows, e->d_po_states, rows, e->d_po_counts, rows * 2)) return rc;
    }
    int32_t *d_wins = e->d_po_counts, *d_losses = e->d_po_counts + n;
    HIP_TRY(hipMemcpyAsync(e->d_po_states, states, sizeof(uttt_state_t) * (size_t)n, hipMemcpyHostToDevice, e->stream));
    timed_launch(e, kKPlayout, k_playout_states, dim3(grid_waves(n)), dim3(kBlock), (const uttt_state_t *)e->d_po_states.get(),
                 (int)n, (int)playouts, seed, d_wins, d_losses);
    if (int rc = check_launch()) return rc;
    HIP_TRY(hipMemcpyAsync(wins, d_wins, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipMemcpyAsync(losses, d_losses, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    drain_events(e);
    return UTTT_OK;
}

int uttt_solve(uttt_engine_t *e, const uttt_state_t *states, int64_t n, int32_t max_nodes, int8_t *value,
               int8_t *action, int8_t *status, int64_t *nodes, int8_t *action_values) {
    if (!e) return UTTT_ERR_ARG;
    if (int rc = solve_check_args("uttt_solve", states, n, max_nodes)) return rc;
    if (n == 0) return UTTT_OK;
    HIP_TRY(hipSetDevice(e->device));
    if (n > e->sv_rows) {
        int64_t rows = e->sv_rows ? e->sv_rows : 1024;
        while (rows < n) rows *= 2;
        if (int rc = grow_group(e->sv_rows, rows, e->d_sv_states, rows, e->d_sv_out, rows * 84, e->d_sv_nodes, rows))
            return rc;
    }
    int8_t *d_value = e->d_sv_out, *d_action = d_value + n, *d_status = d_action + n, *d_av = d_status + n;
    HIP_TRY(hipMemcpyAsync(e->d_sv_states, states, sizeof(uttt_state_t) * (size_t)n, hipMemcpyHostToDevice, e->stream));
    timed_launch(e, kKSolve, k_solve_states, dim3(grid_waves((int)n)), dim3(kBlock),
                 (const uttt_state_t *)e->d_sv_states.get(), (int)n, max_nodes, d_value, d_action, d_status,
                 e->d_sv_nodes.get(), d_av);
    if (int rc = check_launch()) return rc;
    const auto out = [&](void *dst, const void *src, size_t bytes) {
        return dst ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, e->stream) : hipSuccess;
    };
    HIP_TRY(out(value, d_value, (size_t)n));
    HIP_TRY(out(action, d_action, (size_t)n));
    HIP_TRY(out(status, d_status, (size_t)n));
    HIP_TRY(out(nodes, e->d_sv_nodes.get(), sizeof(int64_t) * (size_t)n));
    HIP_TRY(out(action_values, d_av, (size_t)n * 81));
    HIP_TRY(hipStreamSynchronize(e->stream));
    drain_events(e);
    return UTTT_OK;
}

int uttt_eval_solve_dev(uttt_engine_t *e, int32_t max_empties, int32_t max_nodes, int32_t priors, float *policy,
                        int64_t policy_ld, float *value, int64_t value_ld, int8_t *status) {
    if (!e) return UTTT_ERR_ARG;
    if (int rc = overlay_check_args("uttt_eval_solve_dev", max_empties, max_nodes, priors, policy, policy_ld, value,
                                    value_ld))
        return rc;
    HIP_TRY(hipSetDevice(e->device));
    timed_launch(e, kKSolveLeaves, k_solve_leaves, dim3(grid_waves(e->tr.n_trees)), dim3(kBlock), e->tr, max_empties,
                 max_nodes, priors, policy, policy_ld, value, value_ld, status);
    return check_launch();
}

int uttt_sym_pending_dev(uttt_engine_t *e, int32_t mode, uint64_t g_or_seed, uttt_state_t *states_out, int8_t *sym_out,
                         float *nn_input_out) {
    if (!e || !states_out || !sym_out) {
        set_error("uttt_sym_pending_dev: null engine, states_out or sym_out");
        return UTTT_ERR_ARG;
    }
    if (mode != UTTT_SYM_FIXED && mode != UTTT_SYM_HASHED) {
        set_error("mode must be UTTT_SYM_FIXED (0) or UTTT_SYM_HASHED (1) (got %d)", mode);
        return UTTT_ERR_ARG;
    }
    if (mode == UTTT_SYM_FIXED && g_or_seed >= (uint64_t)kSymCount) {
        set_error("a fixed symmetry must be 0..%d (got %llu)", kSymCount - 1, (unsigned long long)g_or_seed);
        return UTTT_ERR_ARG;
    }
    HIP_TRY(hipSetDevice(e->device));
    timed_launch(e, kKSymLeaves, k_sym_leaves, dim3(grid_waves(e->tr.n_trees)), dim3(kBlock), e->tr, mode, g_or_seed,
                 states_out, sym_out, nn_input_out);
    return check_launch();
}

// [a, a + rows * ld) and [b, b + rows * ld_b) share a float
static bool rows_overlap(const float *a, int64_t ld_a, const float *b, int64_t ld_b, int64_t rows) {
    return a < b + rows * ld_b && b < a + rows * ld_a;
}

int uttt_sym_rows_dev(uttt_engine_t *e, const int8_t *sym, const float *policy, int64_t policy_ld, const float *value,
                      int64_t value_ld, float *out_policy, int64_t out_policy_ld, float *out_value,
                      int64_t out_value_ld, int32_t accumulate, float scale) {
    if (!e || !sym || !policy || !value || !out_policy || !out_value) {
        set_error("uttt_sym_rows_dev: null pointer");
        return UTTT_ERR_ARG;
    }
    if (policy_ld < 81 || out_policy_ld < 81) {
        set_error("policy_ld must be at least 81 (got %lld and %lld)", (long long)policy_ld, (long long)out_policy_ld);
        return UTTT_ERR_ARG;
    }
    if (value_ld < 1 || out_value_ld < 1) {
        set_error("value_ld must be at least 1 (got %lld and %lld)", (long long)value_ld, (long long)out_value_ld);
        return UTTT_ERR_ARG;
    }
    // the kernel reads and writes at most one row per tree of the search: over that many rows no output may
    // share a float with an input (a value column may lie inside its own policy's padding, not the other's)
    const int64_t rows = e->tr.n_trees > 0 ? e->tr.n_trees : 1;
    if (rows_overlap(policy, policy_ld, out_policy, out_policy_ld, rows) ||
        rows_overlap(value, value_ld, out_value, out_value_ld, rows) ||
        rows_overlap(policy, policy_ld, out_value, out_value_ld, rows) ||
        rows_overlap(value, value_ld, out_policy, out_policy_ld, rows)) {
        set_error("uttt_sym_rows_dev: the output buffers overlap the input buffers (over %lld rows)", (long long)rows);
        return UTTT_ERR_ARG;
    }
    HIP_TRY(hipSetDevice(e->device));
    timed_launch(e, kKSymRows, k_sym_rows, dim3(grid_waves(e->tr.n_trees)), dim3(kBlock), e->tr, sym, policy, policy_ld,
                 value, value_ld, out_policy, out_policy_ld, out_value, out_value_ld, accumulate ? 1 : 0, scale);
    return check_launch();
}

static bool fused_rounds() {  // k_round1 (UTTT_FUSED_ROUNDS=0: the public calls' launches)
    static const bool fuse = [] {
        const char *v = getenv("UTTT_FUSED_ROUNDS");
        return !(v && v[0] == '0');
    }();
    return fuse;
}

// part_host != nullptr (uttt_rounds_hash_move only, with the fused rounds): the round's counts go to per-block
// words instead of the ring slot (k_round1's part_host form)
static int round_hash_async_impl(uttt_engine *e, int32_t ring_slot, int32_t tag, float *policy, float *value,
                                 uint32_t *part_host, uint32_t *part_dev, const uint32_t *part_prev, int nb_prev,
                                 int stats_parity) {
    if (!e || !policy || !value || ring_slot < 0 || ring_slot >= kCountRing) {
        set_error("uttt_round_hash_async: bad arguments (ring slot must be in 0..%d)", kCountRing - 1);
        return UTTT_ERR_ARG;
    }
    if (!fused_rounds()) {
        int rc = select_async_impl(e, e->h_ring + 4 * ring_slot, tag);
        if (rc) return rc;
        if ((rc = uttt_eval_hash_dev(e, policy, value))) return rc;
        return uttt_search_apply(e, policy, 81, value, 1, 0, 1);
    }
    // the whole round in one dispatch (k_round1): the previous round's apply, this round's select and its
    // evaluation, which is staged for the next round
    if (e->phase != 1) {
        set_error("uttt_round_hash_async: call uttt_search_begin (or apply the previous round) first");
        return UTTT_ERR_ORDER;
    }
    HIP_TRY(hipSetDevice(e->device));
    if (e->host_apply_rows) {  // (a one-tree host evaluation cannot be staged beside a round's)
        if (int rc0 = flush_host_apply(e)) return rc0;
    }
    const int apply = e->dev_apply_staged ? 1 : 0;
    timed_launch(e, kKSelect, e->tr.py ? k_round1<true> : k_round1<false>, dim3(grid_waves(e->tr.n_trees)),
                 dim3(kBlock), e->pool, e->tr, e->cache, e->dev_apply_policy, e->dev_apply_value, policy, value, apply,
                 stats_ptr(e), e->h_ring + 4 * ring_slot, tag, e->d_r1ctl.get(), part_host, part_dev,
                 part_prev, nb_prev, stats_parity);
    if (int rc0 = check_launch()) return rc0;
    e->dev_apply_policy = policy;
    e->dev_apply_value = value;
    e->dev_apply_staged = true;
    e->phase = 1;
    e->n_pending = 0;
    return UTTT_OK;
}

int uttt_round_hash_async(uttt_engine_t *e, int32_t ring_slot, int32_t tag, float *policy, float *value) {
    return round_hash_async_impl(e, ring_slot, tag, policy, value, nullptr, nullptr, nullptr, 0, 0);
}

int uttt_rounds_hash_async(uttt_engine_t *e, int32_t ring_slot, int32_t tag, float *policy, float *value,
                           int32_t n_rounds) {
    if (!e || n_rounds < 1 || n_rounds > kCountRing) {
        set_error("uttt_rounds_hash_async: n_rounds must be in 1..%d", kCountRing);
        return UTTT_ERR_ARG;
    }
    for (int32_t i = 0; i < n_rounds; ++i)
        if (int rc = uttt_round_hash_async(e, (ring_slot + i) % kCountRing, tag + i, policy, value)) return rc;
    return UTTT_OK;
}

int uttt_rounds_hash_move(uttt_engine_t *e, int32_t ring_slot, int32_t tag, float *policy, float *value, int32_t depth,
                          int32_t *n_rounds, int64_t *n_leaves, int32_t *n_with_leaves) {
    if (!e || !n_rounds || !n_leaves || !n_with_leaves || depth < 1 || depth >= kCountRing || ring_slot < 0 ||
        ring_slot >= kCountRing) {
        set_error("uttt_rounds_hash_move: bad arguments (depth in 1..%d, ring slot in 0..%d)", kCountRing - 1,
                  kCountRing - 1);
        return UTTT_ERR_ARG;
    }
    // per-block count words (k_round1's part_host form: no last-block publish; the unfused rounds keep the ring
    // slot's counts); with kernel timing, each round folds the previous round's select statistics (rows by
    // round parity) at its start
    const bool parts = fused_rounds();
    const int nb = grid_waves(e->tr.n_trees);
    if (parts && !e->h_part) {
        const int cap = grid_waves(e->max_trees);
        if (int rc = e->h_part.grow((int64_t)kCountRing * cap)) return rc;
        memset(e->h_part, 0xFF, sizeof(uint32_t) * (size_t)kCountRing * cap);  // no word valid (n0 field 31)
        if (int rc = alloc_n(e, e->d_part, (size_t)2 * cap)) {
            e->h_part.reset();  // (the pair is made once, together)
            return rc;
        }
        e->part_cap = cap;
    }
    const int cap = e->part_cap;
    int32_t enq = 0, head = 0, with_leaves = 0;
    int64_t leaves = 0;
    auto tag_of = [tag](int32_t i) { return (int32_t)(((uint32_t)tag + (uint32_t)i) & 0x7FFFFFFFu); };
    auto push = [&]() -> int {
        const int slot = (ring_slot + enq) % kCountRing;
        const int rc = parts ? round_hash_async_impl(e, slot, tag_of(enq), policy, value, e->h_part + (size_t)slot * cap,
                                                     e->d_part + (size_t)(enq & 1) * cap,
                                                     enq ? e->d_part + (size_t)((enq - 1) & 1) * cap : nullptr, nb,
                                                     (e->round_parity++) & 1)
                             : uttt_round_hash_async(e, slot, tag_of(enq), policy, value);
        if (rc == UTTT_OK) ++enq;
        return rc;
    };
    auto finish = [&](int rc) {
        *n_rounds = enq;
        *n_leaves = leaves;
        *n_with_leaves = with_leaves;
        return rc;
    };
    auto wait_counts = [&](auto &&ready) {
        return spin_wait(e, "a hash round's counts", ready,
                         drained_error("engine: a hash round ended without storing its counts"));
    };
    for (int32_t i = 0; i < depth; ++i)
        if (int rc = push()) return finish(rc);
    for (;;) {
        const int slot = (ring_slot + head) % kCountRing;
        const int32_t want = tag_of(head);
        int32_t n = 0, left = 0;
        if (parts) {  // every block's word carries this round's tag: sum them
            const uint32_t *pw = e->h_part + (size_t)slot * cap;
            const uint32_t want17 = (uint32_t)want & kPartTagMask;
            auto word_ok = [&](uint32_t w) { return (w >> kPartTagShift) == want17 && (w & 0x1Fu) <= 16u; };
            int i = 0;  // the words before i have arrived (a word stays until the host has read its round)
            if (int rc = wait_counts([&] {
                    while (i < nb && word_ok(__atomic_load_n(pw + i, __ATOMIC_ACQUIRE))) ++i;
                    return i >= nb;
                }))
                return finish(rc);
            for (int j = 0; j < nb; ++j) {
                const uint32_t w = __atomic_load_n(pw + j, __ATOMIC_ACQUIRE);
                n += (int32_t)(w & 0x1Fu);
                left += (int32_t)((w >> 10) & 0x1Fu);
            }
        } else {
            const int32_t *w = e->h_ring + 4 * slot;
            if (int rc = wait_counts([&] { return __atomic_load_n(w + 3, __ATOMIC_ACQUIRE) == want; })) return finish(rc);
            n = __atomic_load_n(w + 0, __ATOMIC_ACQUIRE);
            left = __atomic_load_n(w + 2, __ATOMIC_ACQUIRE);
        }
        leaves += n;
        with_leaves += n > 0 ? 1 : 0;
        ++head;
        if (left <= 0) {  // the move's last round: the ones behind it are empty
            // a round enqueued behind it applied its leaves and queued none, so the evaluation staged by the
            // last enqueued round is empty: the move end need not flush it (one k_apply_tree launch less)
            if (enq > head) e->dev_apply_staged = false;
            return finish(UTTT_OK);
        }
        if (int rc = push()) return finish(rc);
    }
}

static int check_tree_errors(uttt_engine *e) {
    std::vector<TreeCtl> ctl(e->tr.n_trees);
    HIP_TRY(hipMemcpyAsync(ctl.data(), e->tr.ctl, sizeof(TreeCtl) * e->tr.n_trees, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    for (int t = 0; t < e->tr.n_trees; ++t) {
        if (ctl[t].status & kErrMask) {
            set_error("tree %d failed (status 0x%x: %s)", t, ctl[t].status, tree_error_text((uint32_t)ctl[t].status));
            return tree_error_code((uint32_t)ctl[t].status);
        }
    }
    return UTTT_OK;
}

// Before a search's root results are read: a staged evaluation applied, then any failed tree reported
static int root_results_ready(uttt_engine *e) {
    if (!e) return UTTT_ERR_ARG;
    HIP_TRY(hipSetDevice(e->device));
    if (int rc = flush_host_apply(e)) return rc;
    return check_tree_errors(e);
}

int uttt_search_root_visits(uttt_engine_t *e, int32_t *visits, int32_t *n_legal) {
    int rc = root_results_ready(e);
    if (rc) return rc;
    const int n = e->tr.n_trees;
    hipLaunchKernelGGL(k_root_visits, dim3((n * 81 + 255) / 256), dim3(256), 0, e->stream, e->pool, e->tr,
                       e->d_visits.get(), e->d_nlegal.get());
    if ((rc = check_launch())) return rc;
    if (visits)
        HIP_TRY(hipMemcpyAsync(visits, e->d_visits, sizeof(int32_t) * 81 * n, hipMemcpyDeviceToHost, e->stream));
    if (n_legal) HIP_TRY(hipMemcpyAsync(n_legal, e->d_nlegal, sizeof(int32_t) * n, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return UTTT_OK;
}

int uttt_search_scores(uttt_engine_t *e, float temperature, float *scores, int32_t *n_legal) {
    int rc = root_results_ready(e);
    if (rc) return rc;
    const int n = e->tr.n_trees;
    hipLaunchKernelGGL(k_root_scores, dim3((n + 255) / 256), dim3(256), 0, e->stream, e->pool, e->tr, temperature,
                       e->d_scores.get(), e->d_nlegal.get());
    if ((rc = check_launch())) return rc;
    if (scores) HIP_TRY(hipMemcpyAsync(scores, e->d_scores, sizeof(float) * 81 * n, hipMemcpyDeviceToHost, e->stream));
    if (n_legal) HIP_TRY(hipMemcpyAsync(n_legal, e->d_nlegal, sizeof(int32_t) * n, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return UTTT_OK;
}

int uttt_search_root_priors(uttt_engine_t *e, float *priors, int32_t *n_legal) {
    int rc = root_results_ready(e);
    if (rc) return rc;
    const int n = e->tr.n_trees;
    if (n <= 0) {
        set_error("uttt_search_root_priors: no search has begun");
        return UTTT_ERR_ORDER;
    }
    hipLaunchKernelGGL(k_root_priors, dim3((n * 81 + 255) / 256), dim3(256), 0, e->stream, e->pool, e->tr,
                       e->d_scores.get(), e->d_nlegal.get());
    if ((rc = check_launch())) return rc;
    if (priors) HIP_TRY(hipMemcpyAsync(priors, e->d_scores, sizeof(float) * 81 * n, hipMemcpyDeviceToHost, e->stream));
    if (n_legal) HIP_TRY(hipMemcpyAsync(n_legal, e->d_nlegal, sizeof(int32_t) * n, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return UTTT_OK;
}

int uttt_engine_set_root_noise(uttt_engine_t *e, float epsilon, float alpha, uint64_t seed) {
    if (!e) return UTTT_ERR_ARG;
    if (int rc = noise_check_args("uttt_engine_set_root_noise", epsilon, alpha)) return rc;
    e->noise_eps = epsilon;
    e->noise_alpha = alpha;
    e->noise_seed = seed;
    return UTTT_OK;
}

// ------------------------------------------------------------- tree reuse --
// k_reroot in place of k_begin: the failure flag zeroed on the stream first (a wave of k_reroot may raise it, so the
// kernel cannot reset it itself as k_begin does), the launch, and the two pools changing places
static int launch_reroot(uttt_engine *e, int n, const RerootSrc &src, unsigned long long *err) {
    HIP_TRY(hipMemsetAsync(e->tr.count + 3, 0, sizeof(int32_t), e->stream));
    timed_launch(e, kKReroot, k_reroot, dim3(grid_waves(n)), dim3(kBlock), e->pool, e->pool2, e->tr, src, err);
    std::swap(e->pool.rec, e->pool2.rec);
    return UTTT_OK;
}

int uttt_engine_set_tree_reuse(uttt_engine_t *e, int32_t on) {
    if (!e) return UTTT_ERR_ARG;
    // (any time: the setting is read when a move begins, and the pool then holds the last ended move's trees
    // whichever kernel built their roots)
    HIP_TRY(hipSetDevice(e->device));
    if (on && !e->m_rec2) {  // the to-space: as large as the node pool, kept once it is there
        if (int rc = alloc_n(e, e->m_rec2, (size_t)e->max_trees * (size_t)e->cap, &e->pool2.rec)) return rc;
        e->pool2.cap = e->cap;
    }
    e->tree_reuse = on != 0;
    return UTTT_OK;
}

int uttt_search_reroot(uttt_engine_t *e, const int32_t *actions, int32_t evaluate_count) {
    if (!e || !actions) return UTTT_ERR_ARG;
    if (!e->tree_reuse) {
        set_error("uttt_search_reroot: tree reuse is off (uttt_engine_set_tree_reuse)");
        return UTTT_ERR_ORDER;
    }
    if (e->selfplay || e->tr.n_trees <= 0 || e->phase != 1) {
        set_error("uttt_search_reroot: needs a search begun by uttt_search_begin whose leaves are all applied");
        return UTTT_ERR_ORDER;
    }
    if (e->tr.py) {
        set_error("uttt_search_reroot: the search has Python semantics (its expansions replace): C++ semantics only");
        return UTTT_ERR_ARG;
    }
    if (evaluate_count < e->tr.sims || evaluate_count > e->max_sims) {
        set_error("uttt_search_reroot: evaluate_count %d out of range %d (the finished search's) .. %d (engine max_sims)",
                  evaluate_count, e->tr.sims, e->max_sims);
        return UTTT_ERR_ARG;
    }
    HIP_TRY(hipSetDevice(e->device));
    if (int rc = search1_stop(e)) return rc;
    if (int rc = flush_host_apply(e)) return rc;
    if (int rc = check_tree_errors(e)) return rc;
    const int n = e->tr.n_trees;
    std::vector<uttt_state_t> roots((size_t)n);
    HIP_TRY(hipMemcpyAsync(roots.data(), e->tr.root, sizeof(uttt_state_t) * n, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    for (int t = 0; t < n; ++t) {
        uint32_t m[3];
        legal_mask(roots[t], m);
        if (actions[t] < 0 || actions[t] > 80 || !bit_of(m, actions[t])) {
            set_error("uttt_search_reroot: action %d is not a legal move of tree %d's root", actions[t], t);
            return UTTT_ERR_ARG;
        }
    }
    if (int rc = e->d_actions.grow(e->max_trees)) return rc;
    HIP_TRY(hipMemcpyAsync(e->d_actions, actions, sizeof(int32_t) * n, hipMemcpyHostToDevice, e->stream));
    e->tr.sims = evaluate_count;
    const RerootSrc src{nullptr, nullptr, nullptr, e->d_actions.get(), 0};
    if (int rc = launch_reroot(e, n, src, nullptr)) return rc;
    launch_root_noise(e, nullptr, 0);
    if (int rc = check_launch()) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));  // the caller's actions were read
    e->phase = 1;
    e->n_pending = 0;
    return UTTT_OK;
}

int uttt_search_tree(uttt_engine_t *e, int32_t tree, uint32_t *records, int32_t cap, int32_t *node_count) {
    if (!e || !node_count || tree < 0 || tree >= e->tr.n_trees || (records && cap < 0)) {
        set_error("uttt_search_tree: bad arguments (tree %d of %d)", tree, e ? e->tr.n_trees : 0);
        return UTTT_ERR_ARG;
    }
    HIP_TRY(hipSetDevice(e->device));
    if (int rc = flush_host_apply(e)) return rc;
    TreeCtl ctl;
    HIP_TRY(hipMemcpyAsync(&ctl, e->tr.ctl + tree, sizeof(ctl), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    *node_count = ctl.node_count;
    if (!records) return UTTT_OK;
    if (ctl.node_count < 0 || ctl.node_count > e->cap || cap < ctl.node_count) {
        set_error("uttt_search_tree: the tree has %d records, room for %d", ctl.node_count, cap);
        return UTTT_ERR_ARG;
    }
    HIP_TRY(hipMemcpyAsync(records, e->pool.rec + (size_t)tree * e->pool.cap, sizeof(uint4) * (size_t)ctl.node_count,
                           hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return UTTT_OK;
}

// ------------------------------------------------------------------ match --
}  // extern "C"

// A match's memory has the engine's one-owner buffers: `delete m` frees every block
struct uttt_match {
    int device = 0;
    int max_games = 0;
    hipStream_t stream = nullptr;
    Match mt{};  // what the kernels take by value: raw pointers, filled from the owners below
    DevBuf<uttt_state_t> d_state, d_roots;
    DevBuf<int32_t> d_ply, d_list;
    DevBuf<int8_t> d_action, d_result;
    PinBuf<int64_t> h_counts;  // k_match_lists' five counters
    bool begun = false;
    bool have_counts = false;        // uttt_match_counts has read the counters of the last k_match_lists
    bool moved[2] = {false, false};  // the player has moved since the last k_match_lists: its list is stale
    uttt_engine *searching[2] = {nullptr, nullptr};  // the engine whose search uttt_match_search_begin began
    int64_t counts[5] = {0, 0, 0, 0, 0};
};

static int match_player_check(const char *fn, uttt_match *m, uttt_engine *e, int32_t player) {
    if (!m || !e || (player != 0 && player != 1)) {
        set_error("%s: null match or engine, or a player other than 0 and 1", fn);
        return UTTT_ERR_ARG;
    }
    if (!m->begun) {
        set_error("%s: call uttt_match_begin first", fn);
        return UTTT_ERR_ORDER;
    }
    if (e->device != m->device || e->stream != m->stream) {
        set_error("%s: the engine runs on another device or stream than the match (uttt_engine_set_stream)", fn);
        return UTTT_ERR_ARG;
    }
    return UTTT_OK;
}

static int launch_match_lists(uttt_match *m) {
    hipLaunchKernelGGL(k_match_lists, dim3(1), dim3(1024), 0, m->stream, m->mt, m->h_counts.get());
    m->have_counts = false;
    m->moved[0] = m->moved[1] = false;
    m->searching[0] = m->searching[1] = nullptr;
    return check_launch();
}

extern "C" {

int uttt_match_create(int32_t device, int32_t max_games, uttt_match_t **out) {
    if (!out || max_games < 1 || max_games > kMatchMaxGames) {
        set_error("uttt_match_create: bad arguments (max_games=%d of at most %d)", max_games, kMatchMaxGames);
        return UTTT_ERR_ARG;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        set_error("no HIP device visible");
        return UTTT_ERR_NODEVICE;
    }
    if (device < 0 && hipGetDevice(&device) != hipSuccess) device = 0;
    if (device < 0 || device >= ndev) {
        set_error("device %d out of range (%d visible)", device, ndev);
        return UTTT_ERR_NODEVICE;
    }
    HIP_TRY(hipSetDevice(device));
    uttt_match *m = new uttt_match();
    m->device = device;
    m->max_games = max_games;
    const int64_t n = max_games;
    int rc = UTTT_OK;
    if ((rc = m->d_state.grow(n)) || (rc = m->d_roots.grow(2 * n)) || (rc = m->d_ply.grow(n)) ||
        (rc = m->d_list.grow(2 * n)) || (rc = m->d_action.grow(n * kMaxPlies)) || (rc = m->d_result.grow(n)) ||
        (rc = m->h_counts.grow(5))) {
        delete m;
        return rc;
    }
    memset(m->h_counts, 0, 5 * sizeof(int64_t));
    m->mt.state = m->d_state;
    m->mt.roots = m->d_roots;
    m->mt.ply = m->d_ply;
    m->mt.list = m->d_list;
    m->mt.action = m->d_action;
    m->mt.result = m->d_result;
    m->mt.max_games = max_games;
    *out = m;
    return UTTT_OK;
}

int uttt_match_destroy(uttt_match_t *m) {
    if (!m) return UTTT_OK;
    (void)hipSetDevice(m->device);
    if (m->begun) (void)hipStreamSynchronize(m->stream);
    delete m;
    return UTTT_OK;
}

int uttt_match_begin(uttt_match_t *m, const uttt_state_t *openings, int32_t n_openings, int32_t games, int32_t paired,
                     int32_t sample_plies, uint64_t seed, void *stream) {
    if (!m) return UTTT_ERR_ARG;
    if (int rc = uttt_match_check_host(openings, n_openings, games, m->max_games, paired)) return rc;
    HIP_TRY(hipSetDevice(m->device));
    if (m->begun) HIP_TRY(hipStreamSynchronize(m->stream));  // an earlier match's kernels, before its memory is rewritten
    m->stream = (hipStream_t)stream;
    m->begun = false;
    std::vector<uttt_state_t> start((size_t)games);
    for (int g = 0; g < games; ++g) start[g] = openings[match_opening_of(g, paired)];
    HIP_TRY(hipMemcpyAsync(m->mt.state, start.data(), sizeof(uttt_state_t) * games, hipMemcpyHostToDevice, m->stream));
    HIP_TRY(hipMemsetAsync(m->mt.ply, 0, sizeof(int32_t) * games, m->stream));
    HIP_TRY(hipMemsetAsync(m->mt.action, 0xFF, (size_t)games * kMaxPlies, m->stream));  // -1
    HIP_TRY(hipMemsetAsync(m->mt.result, 0xFF, (size_t)games, m->stream));              // kMatchLive
    m->mt.games = games;
    m->mt.sample_plies = sample_plies;
    m->mt.seed = seed;
    if (int rc = launch_match_lists(m)) return rc;
    HIP_TRY(hipStreamSynchronize(m->stream));  // `start` was read
    m->begun = true;
    return UTTT_OK;
}

int uttt_match_counts(uttt_match_t *m, int64_t out[5]) {
    if (!m || !out) return UTTT_ERR_ARG;
    if (!m->begun) {
        set_error("uttt_match_counts: call uttt_match_begin first");
        return UTTT_ERR_ORDER;
    }
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(hipStreamSynchronize(m->stream));
    if (!m->moved[0] && !m->moved[1]) {  // (after a move the counters are still the last lists': nothing new to read)
        for (int i = 0; i < 5; ++i) m->counts[i] = __atomic_load_n(m->h_counts.get() + i, __ATOMIC_ACQUIRE);
        m->have_counts = true;
    }
    for (int i = 0; i < 5; ++i) out[i] = m->counts[i];
    return UTTT_OK;
}

int uttt_match_search_begin(uttt_match_t *m, uttt_engine_t *e, int32_t player, int32_t sims, int32_t batch,
                            int32_t semantics) {
    if (int rc = match_player_check("uttt_match_search_begin", m, e, player)) return rc;
    if (int rc = refuse_root_noise(e, "uttt_match_search_begin",
                                   "a plain search keys it by tree index, which a match changes from ply to ply"))
        return rc;
    if (int rc = refuse_tree_reuse(e, "uttt_match_search_begin", "a match's trees change games from ply to ply")) return rc;
    if (!m->have_counts || m->moved[player]) {
        set_error("uttt_match_search_begin: player %d's list is stale (call uttt_match_lists, then uttt_match_counts)",
                  player);
        return UTTT_ERR_ORDER;
    }
    const int64_t n = m->counts[player];
    if (n <= 0) {
        set_error("uttt_match_search_begin: player %d is to move in no live game", player);
        return UTTT_ERR_ARG;
    }
    if (n > e->max_trees) {
        set_error("uttt_match_search_begin: %lld games for an engine of %d trees", (long long)n, e->max_trees);
        return UTTT_ERR_ARG;
    }
    m->searching[player] = nullptr;
    if (int rc = search_begin_roots(e, "uttt_match_search_begin", m->mt.roots + (size_t)player * m->max_games, (int32_t)n,
                                    sims, batch, semantics, hipMemcpyDeviceToDevice))
        return rc;
    m->searching[player] = e;
    return UTTT_OK;
}

int uttt_match_move(uttt_match_t *m, uttt_engine_t *e, int32_t player) {
    if (int rc = match_player_check("uttt_match_move", m, e, player)) return rc;
    if (m->moved[player]) {
        set_error("uttt_match_move: player %d has moved already (call uttt_match_lists)", player);
        return UTTT_ERR_ORDER;
    }
    if (m->searching[player] != e || e->selfplay || e->phase != 1 || e->tr.n_trees != (int32_t)m->counts[player]) {
        set_error("uttt_match_move: needs the search uttt_match_search_begin began on this engine, every leaf applied");
        return UTTT_ERR_ORDER;
    }
    if (int rc = root_results_ready(e)) return rc;
    const int n = e->tr.n_trees;
    hipLaunchKernelGGL(k_root_visits, dim3((n * 81 + 255) / 256), dim3(256), 0, e->stream, e->pool, e->tr,
                       e->d_visits.get(), e->d_nlegal.get());
    if (int rc = check_launch()) return rc;
    hipLaunchKernelGGL(k_match_move, dim3(grid_waves(n)), dim3(kBlock), 0, e->stream, m->mt, (int)player, n,
                       (const int32_t *)e->d_visits.get(), (const int32_t *)e->d_nlegal.get());
    m->moved[player] = true;
    m->searching[player] = nullptr;
    return check_launch();
}

int uttt_match_lists(uttt_match_t *m) {
    if (!m) return UTTT_ERR_ARG;
    if (!m->begun) {
        set_error("uttt_match_lists: call uttt_match_begin first");
        return UTTT_ERR_ORDER;
    }
    HIP_TRY(hipSetDevice(m->device));
    return launch_match_lists(m);
}

int uttt_match_games(uttt_match_t *m, int8_t *results, int32_t *plies, int8_t *actions, uttt_state_t *states) {
    if (!m) return UTTT_ERR_ARG;
    if (!m->begun) {
        set_error("uttt_match_games: call uttt_match_begin first");
        return UTTT_ERR_ORDER;
    }
    HIP_TRY(hipSetDevice(m->device));
    const size_t n = (size_t)m->mt.games;
    if (results) HIP_TRY(hipMemcpyAsync(results, m->mt.result, n, hipMemcpyDeviceToHost, m->stream));
    if (plies) HIP_TRY(hipMemcpyAsync(plies, m->mt.ply, sizeof(int32_t) * n, hipMemcpyDeviceToHost, m->stream));
    if (actions) HIP_TRY(hipMemcpyAsync(actions, m->mt.action, n * kMaxPlies, hipMemcpyDeviceToHost, m->stream));
    if (states) HIP_TRY(hipMemcpyAsync(states, m->mt.state, sizeof(uttt_state_t) * n, hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
    return UTTT_OK;
}

// ----------------------------------------------------------- self-play API --
int uttt_selfplay_set_temperature_schedule(uttt_engine_t *e, int32_t plies, float late_temperature) {
    if (!e) return UTTT_ERR_ARG;
    if (plies < 0 || !(late_temperature >= 0.0f && late_temperature <= 3.0e38f)) {
        set_error("uttt_selfplay_set_temperature_schedule: plies must be >= 0 and late_temperature finite and >= 0 "
                  "(got %d, %g)", plies, (double)late_temperature);
        return UTTT_ERR_ARG;
    }
    if (e->selfplay && e->phase != 0) {
        set_error("uttt_selfplay_set_temperature_schedule: a move is in flight (call it between moves)");
        return UTTT_ERR_ORDER;
    }
    e->sp.temp_plies = plies;
    e->sp.late_temperature = late_temperature;
    return UTTT_OK;
}

int uttt_selfplay_begin(uttt_engine_t *e, int64_t game_begin, int64_t game_end, uint32_t seed_base, float temperature,
                        int32_t sims, int32_t batch, int64_t arena_plies) {
    if (!e || game_end < game_begin || game_begin < 0 || arena_plies <= 0) {
        set_error("uttt_selfplay_begin: bad arguments");
        return UTTT_ERR_ARG;
    }
    HIP_TRY(hipSetDevice(e->device));
    const int slots = e->max_trees;
    int rc = search_begin_common(e, slots, sims, batch);
    e->tr.py = 0;  // self-play is the cpp/uttt_mcts.cpp path
    if (rc) return rc;
    e->phase = 0;  // move_begin first
    e->reuse_ready = false;  // no move of this run has ended: the first k_reroot builds every root fresh
    SelfPlay &sp = e->sp;
    if (!e->m_work) {  // the last of the per-slot blocks: all of them are there, or the run cannot start
        if ((rc = alloc_n(e, e->m_slot, slots, &sp.slot)) || (rc = alloc_n(e, e->m_mt_key, (size_t)slots * 624, &sp.mt_key)) ||
            (rc = alloc_n(e, e->m_mt_pos, slots, &sp.mt_pos)) ||
            (rc = alloc_n(e, e->m_ply_state, (size_t)slots * kMaxPlies, &sp.ply_state)) ||
            (rc = alloc_n(e, e->m_ply_policy, (size_t)slots * kMaxPlies * 81, &sp.ply_policy)) ||
            (rc = alloc_n(e, e->m_ply_action, (size_t)slots * kMaxPlies, &sp.ply_action)) ||
            (rc = alloc_n(e, e->m_ctr, 4, &sp.ctr)) || (rc = alloc_n(e, e->m_live, slots, &sp.live)) ||
            (rc = alloc_n(e, e->m_work, (size_t)slots + 1, &sp.work)))
            return rc;
    }
    // every archived game has >= 1 ply, so the arena bounds the game table too
    const int64_t games = std::max<int64_t>(std::min<int64_t>(game_end - game_begin, arena_plies), 1);
    if (sp.arena_cap < arena_plies) {
        rc = grow_group(sp.arena_cap, arena_plies, e->m_ar_state, arena_plies, e->m_ar_policy, 81 * arena_plies,
                        e->m_ar_action, arena_plies, e->m_ar_value, arena_plies);
        sp.ar_state = e->m_ar_state;  // (null after a failed growth, with arena_cap 0)
        sp.ar_policy = e->m_ar_policy;
        sp.ar_action = e->m_ar_action;
        sp.ar_value = e->m_ar_value;
        if (rc) return rc;
    }
    if (sp.games_cap < games) {
        rc = grow_group(sp.games_cap, games, e->m_games, games);
        sp.games = e->m_games;
        if (rc) return rc;
    }
    sp.game_end = game_end;
    sp.seed_base = seed_base;
    sp.temperature = temperature;
    sp.slots = slots;
    // every slot starts free; k_finalize hands out games [game_begin, ...)
    HIP_TRY(hipMemsetAsync(sp.slot, 0, sizeof(Slot) * slots, e->stream));
    int64_t ctr[4] = {game_begin, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(sp.ctr, ctr, sizeof(ctr), hipMemcpyHostToDevice, e->stream));
    hipLaunchKernelGGL(k_finalize, dim3(1), dim3(1024), 0, e->stream, sp, (const int32_t *)nullptr,
                       (const TreeCtl *)nullptr, (unsigned long long *)nullptr, (int64_t *)nullptr);
    hipLaunchKernelGGL(k_archive, dim3(archive_grid(slots)), dim3(256), 0, e->stream, sp, (const unsigned long long *)nullptr, 1);
    if ((rc = check_launch())) return rc;
    HIP_TRY(hipMemcpyAsync(e->h_move, sp.ctr, sizeof(int64_t) * 4, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->h_move[4] = -1;
    e->selfplay = true;
    e->sp_arena_used = 0;
    e->moves = 0;
    return uttt_engine_cache_clear(e);  // a new run may use a new model
}

// A self-play move's roots: the slots' states, read in place (Slot.state is the first member)
static int launch_move_begin(uttt_engine *e) {
    const int slots = e->sp.slots;
    e->dev_apply_staged = false;  // (a move that was never ended)
    e->host_apply_rows = 0;       // (a one-tree evaluation staged by a search on this engine, never applied)
    e->tr.n_trees = slots;
    e->moves++;
    if (e->tree_reuse) {  // the played moves' subtrees into the other pool, which becomes the trees' pool
        const RerootSrc src{e->sp.slot, e->sp.live, e->sp.ply_action, nullptr, e->reuse_ready ? 0 : 1};
        if (int rc = launch_reroot(e, slots, src, e->d_err.get())) return rc;
    } else {
        hipLaunchKernelGGL(k_begin, dim3(grid_waves(slots)), dim3(kBlock), 0, e->stream, e->pool, e->tr,
                           (const char *)e->sp.slot, (int)sizeof(Slot), (const int32_t *)e->sp.live, e->d_err.get());
    }
    e->reuse_ready = false;  // until this move is ended
    launch_root_noise(e, (const char *)e->sp.slot + offsetof(Slot, game), (int)sizeof(Slot));
    if (int rc = check_launch()) return rc;
    e->phase = 1;
    e->n_pending = 0;
    return UTTT_OK;
}

// A move's end: k_move_end, k_finalize, k_archive. fail / ctl / err / h_move: the asynchronous form's failure
// flag, tree controls, first-failure word and host counters (all null in the blocking form, which has checked
// the trees and copies the counters itself)
static int launch_move_end(uttt_engine *e, const int32_t *fail, const TreeCtl *ctl, unsigned long long *err,
                           int64_t *h_move) {
    const int slots = e->sp.slots;
    {
        TimedLaunch tl(e, kKMoveEnd);
        hipLaunchKernelGGL(k_move_end, dim3(grid_waves(slots)), dim3(kBlock), 0, e->stream, e->pool, e->sp, fail);
        hipLaunchKernelGGL(k_finalize, dim3(1), dim3(1024), 0, e->stream, e->sp, fail, ctl, err, h_move);
        hipLaunchKernelGGL(k_archive, dim3(archive_grid(slots)), dim3(256), 0, e->stream, e->sp,
                           (const unsigned long long *)err, 1);
    }
    e->reuse_ready = true;  // the pool now holds the trees the next move's k_reroot reads
    return check_launch();
}

int uttt_selfplay_move_begin(uttt_engine_t *e, int32_t *n_live) {
    if (!e || !e->selfplay) {
        set_error("uttt_selfplay_move_begin: call uttt_selfplay_begin first");
        return UTTT_ERR_ORDER;
    }
    HIP_TRY(hipSetDevice(e->device));
    const int slots = e->sp.slots;
    if (e->cache.flag && e->cache_clear_every > 0 && e->moves > 0 && e->moves % e->cache_clear_every == 0) {
        int rc0 = uttt_engine_cache_clear(e);
        if (rc0) return rc0;
    }
    std::vector<int32_t> live(slots);
    HIP_TRY(hipMemcpyAsync(live.data(), e->sp.live, sizeof(int32_t) * slots, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    int nl = 0;
    for (int v : live) nl += v != 0;
    if (n_live) *n_live = nl;
    return launch_move_begin(e);
}

int uttt_selfplay_move_end(uttt_engine_t *e, int64_t *n_finished) {
    if (!e || !e->selfplay) {
        set_error("uttt_selfplay_move_end: call uttt_selfplay_begin first");
        return UTTT_ERR_ORDER;
    }
    if (e->phase == 2 || e->phase == 3) {
        set_error("uttt_selfplay_move_end: pending leaves were not applied");
        return UTTT_ERR_ORDER;
    }
    HIP_TRY(hipSetDevice(e->device));
    if (int rc0 = flush_host_apply(e)) return rc0;  // a staged round's evaluation (uttt_round_hash_async)
    int rc = check_tree_errors(e);
    if (rc) return rc;
    if ((rc = launch_move_end(e, nullptr, nullptr, nullptr, nullptr))) return rc;
    int64_t ctr[4];
    HIP_TRY(hipMemcpyAsync(ctr, e->sp.ctr, sizeof(ctr), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    drain_events(e);
    if (ctr[2] > e->sp.arena_cap) {
        set_error("self-play record arena full (%lld plies > %lld)", (long long)ctr[2], (long long)e->sp.arena_cap);
        return UTTT_ERR_CAPACITY;
    }
    e->sp_arena_used = ctr[2];
    if (n_finished) *n_finished = ctr[1];
    e->phase = 0;
    return UTTT_OK;
}

int uttt_selfplay_move_begin_async(uttt_engine_t *e) {
    if (!e || !e->selfplay) {
        set_error("uttt_selfplay_move_begin_async: call uttt_selfplay_begin first");
        return UTTT_ERR_ORDER;
    }
    if (e->phase != 0) {
        set_error("uttt_selfplay_move_begin_async: the previous move was not ended");
        return UTTT_ERR_ORDER;
    }
    if (e->cache.flag && e->cache_clear_every > 0) {
        set_error("uttt_selfplay_move_begin_async: periodic cache clears need the blocking move_begin");
        return UTTT_ERR_ORDER;
    }
    HIP_TRY(hipSetDevice(e->device));
    return launch_move_begin(e);
}

int uttt_selfplay_move_end_async(uttt_engine_t *e) {
    if (!e || !e->selfplay) {
        set_error("uttt_selfplay_move_end_async: call uttt_selfplay_begin first");
        return UTTT_ERR_ORDER;
    }
    if (e->phase != 1) {
        set_error("uttt_selfplay_move_end_async: no move in progress, or pending leaves were not applied");
        return UTTT_ERR_ORDER;
    }
    HIP_TRY(hipSetDevice(e->device));
    if (int rc0 = flush_host_apply(e)) return rc0;  // a staged round's evaluation (uttt_round_hash_async)
    // d_err and the failure flag were reset by this move's k_begin. A failed tree leaves the whole move unended
    // (the failure flag, set where a tree's status gets an error bit; k_finalize then puts the first failed tree
    // into *d_err, which k_archive checks), so the engine is in the state the blocking move end refuses in
    int rc = launch_move_end(e, e->tr.count + 3, e->tr.ctl, e->d_err, e->h_move);
    if (rc) return rc;  // k_finalize stored the counters and the failure word into h_move
    e->phase = 0;
    return UTTT_OK;
}

int uttt_selfplay_move_result(uttt_engine_t *e, int64_t *n_finished, int32_t *n_live_next) {
    if (!e || !e->selfplay) return UTTT_ERR_ORDER;
    const unsigned long long err = (unsigned long long)e->h_move[4];
    if (err != ~0ull) {
        const uint32_t st = (uint32_t)err, t = (uint32_t)(err >> 32);
        set_error("tree %u failed (status 0x%x: %s)", t, st, tree_error_text(st));
        return tree_error_code(st);
    }
    if (e->h_move[2] > e->sp.arena_cap) {
        set_error("self-play record arena full (%lld plies > %lld)", (long long)e->h_move[2],
                  (long long)e->sp.arena_cap);
        return UTTT_ERR_CAPACITY;
    }
    e->sp_arena_used = e->h_move[2];
    drain_events(e);
    if (n_finished) *n_finished = e->h_move[1];
    if (n_live_next) *n_live_next = (int32_t)e->h_move[3];
    return UTTT_OK;
}

int uttt_selfplay_games(uttt_engine_t *e, int64_t *game_ids, int64_t *offsets, int32_t *lengths, int64_t max_games,
                        int64_t *n_games) {
    if (!e || !e->selfplay) return UTTT_ERR_ORDER;
    HIP_TRY(hipSetDevice(e->device));
    int64_t ctr[4];
    HIP_TRY(hipMemcpyAsync(ctr, e->sp.ctr, sizeof(ctr), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    const int64_t n = std::min<int64_t>(ctr[1], e->sp.games_cap);
    std::vector<GameEntry> g((size_t)n);
    if (n) HIP_TRY(hipMemcpy(g.data(), e->sp.games, sizeof(GameEntry) * n, hipMemcpyDeviceToHost));
    std::sort(g.begin(), g.end(), [](const GameEntry &a, const GameEntry &b) { return a.game < b.game; });
    const int64_t m = std::min<int64_t>(n, max_games);
    for (int64_t i = 0; i < m; ++i) {
        if (game_ids) game_ids[i] = g[i].game;
        if (offsets) offsets[i] = g[i].offset;
        if (lengths) lengths[i] = (int32_t)g[i].length;
    }
    if (n_games) *n_games = n;
    return UTTT_OK;
}

int uttt_selfplay_plies(uttt_engine_t *e, uttt_state_t *states, double *policies, int8_t *actions, int8_t *values,
                        float *inputs_hwc, int64_t max_plies, int64_t *n_plies) {
    if (!e || !e->selfplay) return UTTT_ERR_ORDER;
    HIP_TRY(hipSetDevice(e->device));
    const int64_t n = std::min<int64_t>(e->sp_arena_used, max_plies);
    if (n_plies) *n_plies = e->sp_arena_used;
    if (n <= 0) return UTTT_OK;
    if (states) HIP_TRY(hipMemcpy(states, e->sp.ar_state, sizeof(uttt_state_t) * n, hipMemcpyDeviceToHost));
    if (policies) HIP_TRY(hipMemcpy(policies, e->sp.ar_policy, sizeof(double) * 81 * n, hipMemcpyDeviceToHost));
    if (actions) HIP_TRY(hipMemcpy(actions, e->sp.ar_action, n, hipMemcpyDeviceToHost));
    if (values) HIP_TRY(hipMemcpy(values, e->sp.ar_value, n, hipMemcpyDeviceToHost));
    if (inputs_hwc) {
        float *d = nullptr;
        HIP_TRY(hipMalloc((void **)&d, sizeof(float) * 243 * n));
        hipLaunchKernelGGL(k_hwc, dim3((unsigned)((n * 81 + 255) / 256)), dim3(256), 0, e->stream, e->sp.ar_state, n, d);
        hipError_t r = hipGetLastError();
        if (r == hipSuccess) r = hipStreamSynchronize(e->stream);
        if (r == hipSuccess) r = hipMemcpy(inputs_hwc, d, sizeof(float) * 243 * n, hipMemcpyDeviceToHost);
        (void)hipFree(d);
        if (r != hipSuccess) {
            set_error("history tensor expansion failed: %s", hipGetErrorString(r));
            return UTTT_ERR_HIP;
        }
    }
    return UTTT_OK;
}

int uttt_selfplay_get_rng(uttt_engine_t *e, int32_t slot, uint32_t key[624], int32_t *pos) {
    if (!e || !e->selfplay || slot < 0 || slot >= e->sp.slots || !key || !pos) return UTTT_ERR_ARG;
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipMemcpyAsync(key, e->sp.mt_key + (size_t)slot * 624, sizeof(uint32_t) * 624, hipMemcpyDeviceToHost,
                           e->stream));
    HIP_TRY(hipMemcpyAsync(pos, e->sp.mt_pos + slot, sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return UTTT_OK;
}

int uttt_selfplay_set_rng(uttt_engine_t *e, int32_t slot, const uint32_t key[624], int32_t pos) {
    if (!e || !e->selfplay || slot < 0 || slot >= e->sp.slots || !key || pos < 0 || pos > 624) return UTTT_ERR_ARG;
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipMemcpyAsync(e->sp.mt_key + (size_t)slot * 624, key, sizeof(uint32_t) * 624, hipMemcpyHostToDevice,
                           e->stream));
    HIP_TRY(hipMemcpyAsync(e->sp.mt_pos + slot, &pos, sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return UTTT_OK;
}

// ------------------------------------------------------- evaluation cache --
int uttt_engine_set_cache(uttt_engine_t *e, int32_t log2_capacity, int32_t clear_every_moves) {
    if (!e || log2_capacity < 0 || log2_capacity > 26 || clear_every_moves < 0) {
        set_error("uttt_engine_set_cache: log2_capacity must be 0 (off) .. 26");
        return UTTT_ERR_ARG;
    }
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->stream));
    // this engine's own table goes (a shared one is only a view: nothing to free)
    e->bytes -= (int64_t)((sizeof(uint32_t) + kRecBytes) * (size_t)e->m_cache_flag.cap());
    e->m_cache_flag.reset();
    e->m_cache_rec.reset();
    e->cache = EvalCache{};
    e->cache_owner = true;
    e->cache_log2 = 0;
    e->cache_clear_every = clear_every_moves;
    if (log2_capacity == 0) return UTTT_OK;
    int64_t cap = 0;
    if (int rc = grow_group(cap, (int64_t)1 << log2_capacity, e->m_cache_flag, (int64_t)1 << log2_capacity,
                            e->m_cache_rec, (int64_t)kRecBytes << log2_capacity))
        return rc;
    e->cache_log2 = log2_capacity;
    e->bytes += (int64_t)((sizeof(uint32_t) + kRecBytes) * (size_t)cap);
    e->cache.flag = e->m_cache_flag;
    e->cache.rec = e->m_cache_rec;
    e->cache.mask = (uint32_t)(cap - 1);
    e->cache.ctr = e->d_cache_ctr;
    return uttt_engine_cache_clear(e);
}

int uttt_engine_share_cache(uttt_engine_t *e, uttt_engine_t *owner) {
    if (!e || !owner || e == owner || !owner->cache_owner || e->device != owner->device) {
        set_error("uttt_engine_share_cache: need a distinct owner engine (with its own table) on the same device");
        return UTTT_ERR_ARG;
    }
    int rc = uttt_engine_set_cache(e, 0, 0);  // drop this engine's own table
    if (rc) return rc;
    e->cache = owner->cache;
    e->cache.ctr = e->d_cache_ctr;  // statistics stay per engine
    e->cache_log2 = owner->cache_log2;
    e->cache_clear_every = 0;       // only the owner clears
    e->cache_owner = false;
    return UTTT_OK;
}

int uttt_engine_cache_clear(uttt_engine_t *e) {
    if (!e) return UTTT_ERR_ARG;
    if (!e->cache.flag || !e->cache_owner) return UTTT_OK;
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipMemsetAsync(e->cache.flag, 0, sizeof(uint32_t) * ((size_t)1 << e->cache_log2), e->stream));
    // engines sharing the table launch on their own streams: nothing would order their next
    // lookups after this clear, so it completes before the call returns (once per run)
    HIP_TRY(hipStreamSynchronize(e->stream));
    return UTTT_OK;
}

int uttt_engine_cache_stats(uttt_engine_t *e, int64_t *hits, int64_t *misses, int64_t *inserts) {
    return uttt_engine_cache_stats2(e, hits, misses, inserts, nullptr);
}

int uttt_engine_cache_stats2(uttt_engine_t *e, int64_t *hits, int64_t *misses, int64_t *inserts,
                             int64_t *replacements) {
    if (!e) return UTTT_ERR_ARG;
    HIP_TRY(hipSetDevice(e->device));
    static thread_local unsigned long long raw[4 * kRow];
    HIP_TRY(hipMemcpyAsync(raw, e->d_cache_ctr, sizeof(raw), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    unsigned long long c[4] = {0ull, 0ull, 0ull, 0ull};
    for (int k = 0; k < 4; ++k)
        for (int i = 0; i < kStripes; ++i) c[k] += raw[k * kRow + i * kStripeStride];
    if (hits) *hits = (int64_t)c[0];
    if (misses) *misses = (int64_t)c[1];
    if (inserts) *inserts = (int64_t)c[2];
    if (replacements) *replacements = (int64_t)c[3];
    return UTTT_OK;
}

// -------------------------------------------------------------- telemetry --
int uttt_engine_set_timing(uttt_engine_t *e, int32_t enabled) {
    if (!e) return UTTT_ERR_ARG;
    e->timing = enabled != 0;
    return UTTT_OK;
}

int uttt_engine_kernel_stats(uttt_engine_t *e, int32_t kernel, double *total_ms, int64_t *launches, int64_t *bytes) {
    if (!e || kernel < 0 || kernel >= kKernelCount) return UTTT_ERR_ARG;
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->stream));
    drain_events(e);
    unsigned long long b[kRow];
    HIP_TRY(hipMemcpy(b, e->d_bytes + (size_t)kernel * kRow, sizeof(b), hipMemcpyDeviceToHost));
    unsigned long long sum = 0ull;
    for (int i = 0; i < kStripes; ++i) sum += b[i * kStripeStride];
    if (total_ms) *total_ms = e->ms[kernel];
    if (launches) *launches = e->launches[kernel];
    if (bytes) *bytes = (int64_t)sum;
    return UTTT_OK;
}

#ifdef UTTT_DIAG_BUILD
// Diagnostics engine build only: k_select's phase cycles (SelClock) summed over the first kSelDiagTrees
// trees, out[2 * kSpCount + 2]; reset zeroes them.
// the last k_select launch's per-tree wall-clock stamps (g_sel_rt): out[tree * 4 + {start, first root
// done, end, trips}], n_trees entries
int uttt_diag_select_pretouch(int32_t mode) {
    if (mode < 0 || mode > 3) return UTTT_ERR_ARG;
    return hipMemcpyToSymbol(HIP_SYMBOL(g_sel_pretouch), &mode, sizeof(mode)) == hipSuccess ? UTTT_OK : UTTT_ERR_HIP;
}

int uttt_diag_select_rt(unsigned long long *out, int32_t n_trees) {
    static unsigned long long host[kSelDiagTrees][4];
    if (!out || n_trees < 0 || n_trees > kSelDiagTrees) return UTTT_ERR_ARG;
    if (hipMemcpyFromSymbol(host, HIP_SYMBOL(g_sel_rt), sizeof(host)) != hipSuccess) return UTTT_ERR_HIP;
    memcpy(out, host, sizeof(unsigned long long) * 4 * (size_t)n_trees);
    return UTTT_OK;
}

int uttt_diag_select_cycles(unsigned long long *out, int32_t reset) {
    static unsigned long long host[kSelDiagTrees][2 * kSpCount + 2];
    if (out) {
        if (hipMemcpyFromSymbol(host, HIP_SYMBOL(g_sel_cyc), sizeof(host)) != hipSuccess) return UTTT_ERR_HIP;
        for (int j = 0; j < 2 * kSpCount + 2; ++j) {
            out[j] = 0ull;
            for (int t = 0; t < kSelDiagTrees; ++t) out[j] += host[t][j];
        }
    }
    if (reset) {
        memset(host, 0, sizeof(host));
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_sel_cyc), host, sizeof(host)) != hipSuccess) return UTTT_ERR_HIP;
    }
    return UTTT_OK;
}
#endif

int uttt_engine_reset_stats(uttt_engine_t *e) {
    if (!e) return UTTT_ERR_ARG;
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->stream));
    drain_events(e);
    for (int k = 0; k < kKernelCount; ++k) {
        e->ms[k] = 0.0;
        e->launches[k] = 0;
    }
    HIP_TRY(hipMemsetAsync(e->d_bytes, 0, sizeof(unsigned long long) * kKernelCount * kRow, e->stream));
    HIP_TRY(hipMemsetAsync(e->d_cache_ctr, 0, sizeof(unsigned long long) * 4 * kRow, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return UTTT_OK;
}

}  // extern "C"
