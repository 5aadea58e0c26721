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
// One translation unit. What every kernel below builds on lives in engine/, included here in this order:
//   layout.h  errors, HIP_TRY, constants, KernelId, TreeCtl / LeafRec / HostLeaf / Pool / Trees, node records
//   wave.h    lane / wave helpers, DPP arg-max, host-visible stores
//   cache.h   EvalCache: probe, lookup, insert
//   expand.h  legal masks, f32 sums, expand_backup, init_root, k_begin
//   symmetry.h  k_sym_leaves, k_sym_rows: the pending leaves through a symmetry, the rows mapped back
// and, behind the last kernel defined here:
//   noise.h   k_root_noise, k_root_priors: Dirichlet noise mixed into the roots' priors, the priors read back
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

namespace uttt {

// --------------------------------------------------------------- select --
// One wave per tree. uttt_mcts.cpp:109-127 for the simulations up to (and
// including) the next one that reaches an unexpanded non-terminal leaf.
// Terminal simulations are backed up in place (:115-118). The k-1 further
// simulations the reference spends re-finding the same queued leaf are
// accounted by k.
// A launch lasts as long as its slowest tree's chain of dependent loads, and a tree
// whose simulations end on terminals or evaluation-cache hits completes them in place,
// one descent after another. A tree stops after kSelectBudget such completions
// (pending = 2) and resumes in the next launch from the same point: the sequence of
// simulations per tree, hence every result, is unchanged; only the tail of the launch is cut.
constexpr int kSelectBudget = 8;
constexpr int kScanGroup = 4;  // child-scan iterations (64 children each) whose loads are issued together

// k_select phase clock. Product build: empty (every call compiles to nothing). Diagnostics engine
// build (-DUTTT_DIAG_BUILD, libuttt_engine_diag.so, tools/diag/select_cycles.py): each mark drains the
// wave's memory counters, reads s_memtime and charges the cycles since the previous mark to one phase;
// at the end lane 0 adds the wave's phases into g_sel_cyc (all trees, and separately the trees with at
// least kSelHeavyTrips dependent round trips in the launch: the ones that set its length).
enum SelPhase {
    kSpRoot = 0,    // the descent's root link and visits (load wait)
    kSpLoad,        // a child-scan group's loads (wait)
    kSpPuct,        // PUCT values and the per-lane strict '>' scan
    kSpArgmax,      // wave arg-max, winner's registers
    kSpNext,        // next_state, path bookkeeping
    kSpLeaf,        // is_lose / legal count of the leaf
    kSpTerminal,    // terminal backup + fence
    kSpProbe,       // evaluation-cache probe, payload, re-check
    kSpExpand,      // expand + backup of a cache hit (prior sum, child blocks, path)
    kSpHitTail,     // fence + counters after a hit
    kSpQueue,       // pending-leaf record
    kSpRootState,   // the tree's root state (once per launch, before the first descent)
    kSpCount
};
#ifdef UTTT_DIAG_BUILD
constexpr int kSelHeavyTrips = 24;
// per tree (plain read-modify-writes by the tree's own wave: no same-address atomics, which would
// serialize thousands of waves and distort the very latencies measured): [all launches' phases]
// [heavy launches' phases][launches, heavy launches]
constexpr int kSelDiagTrees = 8192;
__device__ unsigned long long g_sel_cyc[kSelDiagTrees][2 * kSpCount + 2];
// the last launch's wall-clock stamps per tree (s_memrealtime, a chip-wide 100 MHz counter): the wave's
// start (its control loads served), its first root phase done, its end; trips in the launch
__device__ unsigned long long g_sel_rt[kSelDiagTrees][4];
// what a live tree's wave loads (and waits for) before its clock starts: 0 nothing, 1 the record 8 past
// its root (another 128-B line of the same page), 2 its root record itself, 3 the record half a pool away
__device__ int g_sel_pretouch;
// the phase sums live in LDS (one row per wave): kept in registers they made k_select spill to
// scratch, whose first accesses are what the diagnostics then measured
__shared__ unsigned long long s_selclk[kWavesPerBlock][kSpCount];
struct SelClock {
    unsigned long long t, rt0, rt1;
    unsigned long long *acc;
    __device__ __forceinline__ void start() {
        acc = s_selclk[threadIdx.x >> 6];
        if ((threadIdx.x & 63) < kSpCount) acc[threadIdx.x & 63] = 0ull;
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        t = __builtin_amdgcn_s_memtime();
        rt0 = __builtin_amdgcn_s_memrealtime();
        rt1 = 0ull;
    }
    template <int P>
    __device__ __forceinline__ void mark() {
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        const unsigned long long n = __builtin_amdgcn_s_memtime();
        if (P == kSpRoot && rt1 == 0ull) rt1 = __builtin_amdgcn_s_memrealtime();
        if ((threadIdx.x & 63) == 0) acc[P] += n - t;
        t = n;
    }
    __device__ __forceinline__ void flush(unsigned int trips) {
        const int tree = (int)(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6));
        if ((threadIdx.x & 63) != 0 || tree >= kSelDiagTrees) return;
        g_sel_rt[tree][0] = rt0;
        g_sel_rt[tree][1] = rt1;
        g_sel_rt[tree][2] = __builtin_amdgcn_s_memrealtime();
        g_sel_rt[tree][3] = trips;
        unsigned long long *row = g_sel_cyc[tree];
        const int h = trips >= (unsigned int)kSelHeavyTrips;
#pragma unroll
        for (int i = 0; i < kSpCount; ++i) {
            row[i] += acc[i];
            if (h) row[kSpCount + i] += acc[i];
        }
        row[2 * kSpCount] += 1ull;
        if (h) row[2 * kSpCount + 1] += 1ull;
    }
};
#else
struct SelClock {
    __device__ __forceinline__ void start() {}
    template <int P>
    __device__ __forceinline__ void mark() {}
    __device__ __forceinline__ void flush(unsigned int) {}
};
#endif

// One scan group of NJ x 64 children of a node (uttt_mcts.cpp:62-78). Every load of the group is
// issued before the first compare (one memory round trip per group; a node expanded by a flush of
// k = 8 copies has up to 8 x 81 children), and each child's link word and visits come with it, so
// the winner's are read from its lane's registers after the arg-max instead of from memory. The PUCT
// values of the group are straight-line code: every child's two correctly rounded divisions are
// independent of every other's, so their latencies overlap instead of running one child after
// another behind per-child branches. Children past cnt (clamped loads) never win; the compare is the
// reference's strict '>' in child order.
// pa >= 0: the previous level's winning action, whose next_state runs while this group's loads are in
// flight (it was on the critical path between the arg-max and the next level's loads)
template <int NJ>
__device__ __forceinline__ void puct_group(const uint4 *__restrict__ R, int first, int c0, int cnt, float sq, int lane,
                                           float &best, int &bi, uint4 &bw, uttt_state_t &s, int &pa, SelClock &clk) {
    uint4 r[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) r[j] = R[first + min(c0 + j * kWave + lane, cnt - 1)];
    if (pa >= 0) {
        s = next_state(s, pa);
        pa = -1;
    }
    clk.mark<kSpLoad>();
    float v[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        // uttt_mcts.cpp:70-72, same association and rounding (no FMA: -ffp-contract=off); the
        // reference divides only when n > 0, and an unvisited child's quotient here is discarded
        const int cn = meta_n(r[j].z);
        const float qd = -__uint_as_float(r[j].x) / (float)max(cn, 1);
        const float q = cn > 0 ? qd : 0.0f;
        const float u = __uint_as_float(r[j].y) * sq / (float)(1 + cn);
        v[j] = q + u;
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int c = c0 + j * kWave + lane;
        const bool take = c < cnt && v[j] > best;
        best = take ? v[j] : best;
        bi = take ? c : bi;
        bw.x = take ? r[j].x : bw.x;  // the winner's record: the back-ups start from it, its meta (visits,
        bw.y = take ? r[j].y : bw.y;  // action, L) and link lead the descent on
        bw.z = take ? r[j].z : bw.z;
        bw.w = take ? r[j].w : bw.w;
    }
    clk.mark<kSpPuct>();
}

// The descent of one tree by one wave (k_select's body; k_flush1 runs it after the previous flush's apply).
// cv_row: this wave's 84-float LDS row (a cache hit's values). host_leaf (one-tree searches only): the
// round's counts, the queued leaf and its copies go to fine-grained host memory behind `tag`, and the
// round's device counts / slot 0 are written here (there is no k_scan launch in that form).
// Returns the tree's pending word (wave-uniform), as stored to tr.pending[t].
template <bool PY>
__device__ __forceinline__ int select_wave(Pool pool, Trees tr, EvalCache cache, unsigned long long *stats, int t,
                                           float *cv_row, HostLeaf *host_leaf, int32_t tag, int max_alt = 0,
                                           uttt_state_t *leaf_out = nullptr) {
    // leaf_out (k_round1): a queued leaf's state as stored to tr.leaf[t], so the caller's evaluation reads it
    // from registers (round 6: a store drain and a reload of tr.leaf[t] ended every tree's round)
    const int lane = lane_id();
    TreeCtl ctl = tr.ctl[t];
    // the root's state and record go out with the control word (round 6: they were a second dependent round
    // trip after the status check; a tree with nothing to do discards them)
    const size_t base = (size_t)t * pool.cap;
    uint4 *__restrict__ R = pool.rec + base;
    const uttt_state_t root = tr.root[t];
    const uint4 root_first = R[0];
    int pend = 0;
    unsigned long long bytes = 0;
    unsigned int levels = 0;
    // cache hits / misses of this tree, counted once at the end: an atomic per hit made the next
    // descent's first load wait for it (vmcnt counts the atomic), ~2k cycles a descent (round 4)
    unsigned int hits = 0, misses = 0;
    // dependent round trips of this wave: the control loads (with the root's state and record), then per
    // descent one per child-scan group, and for a completion in place the cache probe, payload and re-check,
    // the path's read-modify-write and the fence
    unsigned int trips = 1;
    SelClock clk;
#ifdef UTTT_DIAG_BUILD
    if (g_sel_pretouch && (ctl.status & kLive)) {
        const uint4 *pr = pool.rec + (size_t)t * pool.cap;
        const int off = g_sel_pretouch == 1 ? 8 : (g_sel_pretouch == 2 ? 0 : (int)(pool.cap / 2));
        const uint32_t q = pr[off].x;
        asm volatile("s_waitcnt vmcnt(0)" ::"v"(q) : "memory");
    }
#endif
    clk.start();
    if ((ctl.status & kLive) && !(ctl.status & kErrMask) && ctl.sims_done < tr.sims) {
        clk.mark<kSpRootState>();
        int sims_done = ctl.sims_done;
        int budget = tr.budget;
        // the root's record: as loaded with the control word, then after this wave's own last back-up (no
        // other wave writes this tree's nodes during the launch): no descent reloads R[0]
        uint4 root_rec = root_first;
        for (;;) {
            uttt_state_t s = root;
            int node = 0, depth = 0;
            int path_lo = 0, path_hi = 0;  // lane d: path[d], path[64 + d]
            // the current node's meta (visits, action, L) and link (below the root: from the parent's scan)
            const uint4 r0 = root_rec;
            uint2 nm = make_uint2(r0.z, r0.w);
            // lane d: the record of path[d] (prec_lo) and path[64 + d] (prec_hi) as read on the way down
            uint4 prec_lo = r0, prec_hi = make_uint4(0u, 0u, 0u, 0u);
            clk.mark<kSpRoot>();
            bool fail = false;
            int pa = -1;  // a winning action whose next_state is pending (applied under the next loads)
            for (;;) {
                const int cnt = PY ? meta_L(nm.x) : link_k(nm.y) * meta_L(nm.x);
                if (cnt == 0) break;
                const int first = link_first(nm.y);
                const int kself = (node == 0 && !PY) ? 0 : link_k(nm.y);
                const int total = meta_n(nm.x) - kself;  // == sum of children's visits
                int bi = kNone;
                uint4 wr = make_uint4(0u, 0u, 0u, 0u);  // the chosen child's record
                if (!PY) {
                    const float sq = sqrtf((float)total);
                    float best = -1e9f;
                    uint4 bw = make_uint4(0u, 0u, 0u, 0u);
                    // Every load of a group of kScanGroup x 64 children is issued before the first
                    // compare (one memory round trip per group; a node expanded by a flush of k = 8
                    // copies has up to 8 x 81 children), and each child's link word and visits come
                    // with it, so the winner's are read from its lane's registers instead of from
                    // memory after the arg-max: one dependent round trip per level.
                    for (int c0 = 0; c0 < cnt; c0 += kScanGroup * kWave) {
                        ++trips;
                        if (cnt - c0 <= kWave) puct_group<1>(R, first, c0, cnt, sq, lane, best, bi, bw, s, pa, clk);
                        else puct_group<kScanGroup>(R, first, c0, cnt, sq, lane, best, bi, bw, s, pa, clk);
                    }
                    bi = wave_argmax(best, bi, cnt);
                    if (bi != kNone) {  // the winner's lane holds its record
                        const int wl = bi & (kWave - 1);
                        wr = make_uint4((uint32_t)__builtin_amdgcn_readlane((int)bw.x, wl),
                                        (uint32_t)__builtin_amdgcn_readlane((int)bw.y, wl),
                                        (uint32_t)__builtin_amdgcn_readlane((int)bw.z, wl),
                                        (uint32_t)__builtin_amdgcn_readlane((int)bw.w, wl));
                        nm = make_uint2(wr.z, wr.w);
                    }
                    clk.mark<kSpArgmax>();
                } else {
                    trips += 2u + (unsigned int)((cnt + kWave - 1) / kWave);  // the node's record, the scan
                    // pv_mcts.py:120-130 under NumPy 2 promotion: float32 ops with sqrt(t)
                    // in double, or float64 throughout when the priors are float64;
                    // np.argmax: first maximum, a NaN counts as the maximum. (k_apply refuses a
                    // non-finite legal prior or value in both semantics, UTTT_ERR_NONFINITE, where
                    // pv_mcts.py would keep searching, so no NaN statistic reaches this scan today;
                    // the branch keeps the scan a complete restatement of np.argmax)
                    const bool p64 = (nm.x & kMetaP64) != 0u;
                    const double sqt = sqrt((double)total);
                    const float sq = (float)sqt;
                    const double pu = 1.0 / (double)meta_L(nm.x);
                    double best = -HUGE_VAL;
                    for (int c = lane; c < cnt; c += kWave) {
                        const uint4 rc = R[first + c];
                        const int cn = meta_n(rc.z);
                        const float cw = __uint_as_float(rc.x);
                        const bool wf = (rc.z & kMetaWF32) != 0u;
                        double v;
                        if (p64) {
                            const double q = cn > 0 ? (wf ? (double)((-cw) / (float)cn) : (double)(-cw) / (double)cn) : 0.0;
                            v = q + ((1.0 * pu) * sqt) / (double)(1 + cn);
                        } else {
                            const float q = cn > 0 ? (wf ? (-cw) / (float)cn : (float)((double)(-cw) / (double)cn)) : 0.0f;
                            const float u = ((1.0f * __uint_as_float(rc.y)) * sq) / (float)(1 + cn);
                            v = (double)(q + u);
                        }
                        if (v != v) v = HUGE_VAL;
                        if (bi == kNone || v > best) {
                            best = v;
                            bi = c;
                        }
                    }
                    wave_argmax_d(best, bi);
                }
                bi = __builtin_amdgcn_readfirstlane(bi);
                bytes += 12ull * (unsigned long long)cnt + 8ull;
                if (bi == kNone) {  // every child NaN: the reference would dereference null
                    fail = true;
                    if (lane == 0) {
                        ctl.status |= kErrSelect;
                        flag_tree_error(tr);
                    }
                    break;
                }
                node = first + bi;
                ++depth;
                if (depth >= kMaxDepth) {
                    fail = true;
                    if (lane == 0) {
                        ctl.status |= kErrDepth;
                        flag_tree_error(tr);
                    }
                    break;
                }
                if (PY) {
                    wr = R[node];
                    nm = make_uint2(wr.z, wr.w);
                }
                if (lane == (depth & 63)) {
                    if (depth < 64) {
                        path_lo = node;
                        prec_lo = wr;
                    } else {
                        path_hi = node;
                        prec_hi = wr;
                    }
                }
                if (PY) s = next_state(s, meta_action(nm.x));
                else pa = meta_action(nm.x);
                clk.mark<kSpNext>();
            }
            if (pa >= 0) s = next_state(s, pa);  // the leaf's state
            if (fail) break;
            levels += (unsigned int)(depth + 1);
            // the evaluation cache's flags for this leaf are loaded before its terminal checks, which run
            // under that round trip (a terminal leaf's probe is discarded)
            const CacheProbe probe = cache_probe_issue(cache, s);
            const bool lose = is_lose(s);
            const bool no_legal = legal_count(s) == 0u;
            clk.mark<kSpLeaf>();
            if (lose || no_legal) {
                // Terminal: search_leaf returns -(is_lose ? -1 : 0) (uttt_mcts.cpp:19-22),
                // backpropagate adds it at the leaf and flips sign upwards (:47-54).
                const float v = -(lose ? -1.0f : 0.0f);
                auto backup1 = [&](uint4 r, int pn, int d) -> uint4 {  // from the record read on the way down
                    r.x = __float_as_uint(__uint_as_float(r.x) + (((depth - d) & 1) ? -v : v));
                    r.z += 1u;
                    R[pn] = r;
                    return r;
                };
                uint4 nl = prec_lo;
                if (lane <= depth) nl = backup1(prec_lo, path_lo, lane);
                if (lane + 64 <= depth) backup1(prec_hi, path_hi, lane + 64);
                root_rec = make_uint4((uint32_t)__builtin_amdgcn_readlane((int)nl.x, 0),
                                      (uint32_t)__builtin_amdgcn_readlane((int)nl.y, 0),
                                      (uint32_t)__builtin_amdgcn_readlane((int)nl.z, 0),
                                      (uint32_t)__builtin_amdgcn_readlane((int)nl.w, 0));
                wave_memory_fence();
                trips += 2;
                bytes += 16ull * (unsigned long long)(depth + 1);
                clk.mark<kSpTerminal>();
                ++sims_done;
                if (sims_done >= tr.sims) break;
                if (--budget == 0) {
                    pend = 2;
                    break;
                }
                continue;
            }
            // Unexpanded leaf (n == 0 && no children, uttt_mcts.cpp:121): queue it with
            // k = the copies the reference would queue before flushing (:127).
            const int k = min(tr.batch, tr.sims - sims_done);
            float *cv = cv_row;
            trips += cache.flag ? 1 : 0;
            const bool hit = cache_lookup_probed(cache, probe, s, cv);
            clk.mark<kSpProbe>();
            if (hit) {  // the flush's evaluation is already known: apply it now
                trips += 4;
                // cv doubles as the prior sum's row: its values are in registers before the call
                const float h0 = cv[lane], h1 = lane < 17 ? cv[64 + lane] : 0.0f, hv = cv[81];
                const bool hs = !PY && cv[kRecSumFlag] == 1.0f;
                if (!expand_backup(pool, base, node, depth, path_lo, path_hi, prec_lo, prec_hi, k, s, h0, h1, hv,
                                   ctl.node_count, PY, cv, hs, cv[kRecSum], nullptr, &root_rec)) {
                    if (lane == 0) {
                        ctl.status |= kErrCapacity;
                        flag_tree_error(tr);
                    }
                    break;
                }
                clk.mark<kSpExpand>();
                wave_memory_fence();
                ++hits;
                // the probe's flags, the record, the k child blocks and the path's records
                bytes += 32ull + 368ull + 16ull * (unsigned long long)(k * (int)legal_count(s)) + 16ull * (depth + 1);
                clk.mark<kSpHitTail>();
                sims_done += k;
                if (sims_done >= tr.sims) break;
                if (--budget == 0) {
                    pend = 2;
                    break;
                }
                continue;
            }
            misses += cache.flag ? 1u : 0u;
            int32_t *gp = tr.path + (size_t)t * kMaxDepth;
            uint4 *gr = tr.path_rec + (size_t)t * kMaxDepth;
            if (lane <= depth) {
                gp[lane] = path_lo;
                gr[lane] = prec_lo;
            }
            if (lane + 64 <= depth) {
                gp[lane + 64] = path_hi;
                gr[lane + 64] = prec_hi;
            }
            if (lane == 0) {
                LeafRec r;
                r.node = node;
                r.depth = depth;
                r.k = k;
                r.pad = 0;
                tr.rec[t] = r;
                tr.leaf[t] = s;
            }
            if (leaf_out) *leaf_out = s;
            // the probe's flags, the queued path (indices and records), LeafRec and state
            bytes += (cache.flag ? 32ull : 0ull) + 20ull * (unsigned long long)(depth + 1) + 48ull;
            // 3: this leaf's k simulations leave the tree more to do (after its apply)
            pend = (sims_done + k < tr.sims ? 3 : 1) | depth << 8;
            clk.mark<kSpQueue>();
            break;
        }
        ctl.sims_done = sims_done;
        if (lane == 0) tr.ctl[t] = ctl;
    }
    clk.flush(trips);
    if (lane == 0) {
        tr.pending[t] = pend;
        if (hits) atomicAdd(stripe_of(cache.ctr), (unsigned long long)hits);
        if (misses) atomicAdd(stripe_of(cache.ctr + kRow), (unsigned long long)misses);
        if (stats && bytes) atomicAdd(stripe_of(stats + kKSelect * kRow), bytes);
        if (stats && levels) {
            atomicAdd(stripe_of(stats + kKSelLevels * kRow), (unsigned long long)levels);
            atomicAdd(stripe_of(stats + kKSelTrees * kRow), 1ull);
            atomicMax(stripe_of(stats + (max_alt ? kKSelMaxB : kKSelMax) * kRow), (unsigned long long)levels);
            atomicAdd(stripe_of(stats + kKSelTrips * kRow), (unsigned long long)trips);
            atomicMax(stripe_of(stats + (max_alt ? kKSelTripMaxB : kKSelTripMax) * kRow), (unsigned long long)trips);
        }
        if (host_leaf) {  // one tree: what k_scan would derive from pending[0]
            const int p = pend & 0xFF, c0 = (p == 1 || p == 3) ? 1 : 0, c1 = p == 2 ? 1 : 0, c2 = p >= 2 ? 1 : 0;
            tr.count[0] = c0;
            tr.count[1] = c1;
            tr.count[2] = c2;
            tr.tree_of[0] = t;
            tr.depth_of[0] = pend >> 8;
            __hip_atomic_store(&host_leaf->count, c0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(&host_leaf->stopped, c1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(&host_leaf->left, c2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            if (c0) {
                const uttt_state_t st = tr.leaf[t];  // stored by this lane above
                const int32_t *w = reinterpret_cast<const int32_t *>(&st);
                int32_t *d = reinterpret_cast<int32_t *>(&host_leaf->state);
#pragma unroll
                for (int i = 0; i < 8; ++i) __hip_atomic_store(d + i, w[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                __hip_atomic_store(&host_leaf->k, tr.rec[t].k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
            host_stores_done();
            st_host(&host_leaf->tag, tag);
        }
    }
    return __builtin_amdgcn_readfirstlane(pend);
}

template <bool PY>
__global__ __launch_bounds__(kBlock, 4) void k_select(Pool pool, Trees tr, EvalCache cache,
                                                   unsigned long long *stats) {
    __shared__ __attribute__((aligned(16))) float s_hit[kWavesPerBlock][84];  // a cache hit's values, per wave
    const int t = wave_index();
    if (t >= tr.n_trees) return;
    select_wave<PY>(pool, tr, cache, stats, t, s_hit[threadIdx.x >> 6], nullptr, 0);
}

// ------------------------------------------------------------------- scan --
// Exclusive prefix sum of one value per thread over a 1,024-thread block (16 waves): a wave scan
// by lane shifts, the 16 wave totals scanned by the first wave through LDS; two barriers where
// a Hillis-Steele scan over LDS takes twenty. Returns the exclusive prefix; *total gets the sum.
template <typename T>
__device__ __forceinline__ T block_scan_1024(T v, T *total, T *wsum /* __shared__ [16] */) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    T x = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const T t = __shfl_up(x, off);
        if (lane >= off) x += t;
    }
    if (lane == 63) wsum[wave] = x;
    __syncthreads();
    if (wave == 0) {
        T w = lane < 16 ? wsum[lane] : T(0);
#pragma unroll
        for (int off = 1; off < 16; off <<= 1) {
            const T t = __shfl_up(w, off);
            if (lane >= off) w += t;
        }
        if (lane < 16) wsum[lane] = w;
    }
    __syncthreads();
    *total = wsum[15];
    return x - v + (wave > 0 ? wsum[wave - 1] : T(0));
}

// Two exclusive scans over the block in one pass (the barriers and the wave-0 step shared): k_finalize's
// finished lengths and its packed (free, finished) counts (round 6: two passes of block_scan_1024 before)
__device__ __forceinline__ void block_scan2_1024(unsigned long long &a, unsigned long long &c,
                                                 unsigned long long *a_tot, unsigned long long *c_tot,
                                                 unsigned long long *wsum /* __shared__ [32] */) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned long long x = a, y = c;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long tx = __shfl_up(x, off), ty = __shfl_up(y, off);
        if (lane >= off) {
            x += tx;
            y += ty;
        }
    }
    if (lane == 63) {
        wsum[wave] = x;
        wsum[16 + wave] = y;
    }
    __syncthreads();
    if (wave == 0) {
        unsigned long long w = lane < 32 ? wsum[lane] : 0ull;  // lanes 0-15: a's wave sums, 16-31: c's
#pragma unroll
        for (int off = 1; off < 16; off <<= 1) {
            const unsigned long long t = __shfl_up(w, off);
            if ((lane & 15) >= off) w += t;
        }
        if (lane < 32) wsum[lane] = w;
    }
    __syncthreads();
    *a_tot = wsum[15];
    *c_tot = wsum[31];
    a = x - a + (wave > 0 ? wsum[wave - 1] : 0ull);
    c = y - c + (wave > 0 ? wsum[16 + wave - 1] : 0ull);
}

// One block: exclusive scan of pending flags -> tree_of[slot] in tree order.
// host_count (optional): the three counts are also stored to this host-visible (fine-grained pinned)
// word triple at system scope, so the host reads a round's counts when the round's event completes
// without a copy operation on the stream (round 4: one stream operation less per round). Round 5: word 3
// gets the round's tag after them (a system-scope release store), so a host that polls the tag needs no
// event either (uttt_round_hash_async).
__global__ __launch_bounds__(1024) void k_scan(Trees tr, unsigned long long *stats, int32_t *host_count, int32_t tag) {
    __shared__ unsigned long long wsum[16];
    const int tid = threadIdx.x;
    if (stats && tid < 64) {  // the select launch before this scan is complete: fold its slowest tree
        // (the max over the stripes, one per lane of the first wave)
        unsigned long long ml = 0ull, mt = 0ull;
        if (tid < kStripes) {
            unsigned long long *a = stats + kKSelMax * kRow + tid * kStripeStride;
            unsigned long long *b = stats + kKSelTripMax * kRow + tid * kStripeStride;
            ml = *a;
            mt = *b;
            *a = 0ull;
            *b = 0ull;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned long long ol = __shfl_xor(ml, off), ot = __shfl_xor(mt, off);
            ml = ol > ml ? ol : ml;
            mt = ot > mt ? ot : mt;
        }
        if (tid == 0) {
            stats[kKSelMaxSum * kRow] += ml;
            stats[kKSelTripMaxSum * kRow] += mt;
        }
    }
    const int per = (tr.n_trees + 1023) / 1024;
    const int b = tid * per, e = min(b + per, tr.n_trees);
    // up to kScanPer flags per thread (4,096 trees) are loaded together and kept for the second pass (round 5:
    // the two loops each waited for one load per tree in turn); more per thread are re-read there
    constexpr int kScanPer = 4;
    int held[kScanPer];
#pragma unroll
    for (int j = 0; j < kScanPer; ++j) held[j] = b + j < e ? tr.pending[b + j] : 0;
    unsigned long long local = 0, cap = 0, mo = 0;
    for (int i = b; i < e; ++i) {
        const int p = (i - b < kScanPer ? held[i - b] : tr.pending[i]) & 0xFF;
        local += p == 1 || p == 3;
        cap += p == 2;
        mo += p >= 2;
    }
    // the three counts in 21-bit fields of one scanned word (each total <= n_trees < 2^21)
    unsigned long long tot;
    const unsigned long long ex = block_scan_1024(local | (cap << 21) | (mo << 42), &tot, wsum);
    int slot = (int)(ex & 0x1FFFFFull);
    for (int i = b; i < e; ++i) {
        const int p = i - b < kScanPer ? held[i - b] : tr.pending[i];
        if ((p & 1) != 0) {  // 1 or 3
            tr.depth_of[slot] = p >> 8;
            tr.tree_of[slot++] = i;
        }
    }
    if (tid == 0) {
        const int c0 = (int)(tot & 0x1FFFFFull), c1 = (int)((tot >> 21) & 0x1FFFFFull);
        const int c2 = (int)(tot >> 42);  // trees with simulations left after this round (0: the search ends with it)
        tr.count[0] = c0;
        tr.count[1] = c1;
        tr.count[2] = c2;
        if (host_count) {
            __hip_atomic_store(host_count + 0, c0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(host_count + 1, c1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(host_count + 2, c2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            host_stores_done();
            st_host(host_count + 3, tag);
        }
    }
}

// ----------------------------------------------------------------- encode --
// The network input of each pending leaf (uttt_game.cpp:244-280 transposed to
// NCHW as pv_mcts_cpp.py:57-60 does): ch0 own stones, ch1 opponent, ch2 legal.
__global__ __launch_bounds__(256) void k_encode(Trees tr, float *__restrict__ x, int n) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n * 243) return;
    const int slot = g / 243, j = g % 243;
    const int ch = j / 81, pos = j % 81;
    const uttt_state_t s = tr.leaf[tr.tree_of[slot]];
    const int a = action_at(pos);
    uint32_t bit;
    if (ch == 0) bit = bit_of(s.own, a);
    else if (ch == 1) bit = bit_of(s.opp, a);
    else {
        uint32_t m[3];
        legal_mask(s, m);
        bit = bit_of(m, a);
    }
    x[g] = bit ? 1.0f : 0.0f;
}

// ------------------------------------------------------------------ apply --
// One wave per pending leaf (uttt_mcts.cpp:138-167 for each of its k copies):
// legal priors, sequential f32 sum in action order, divide (uniform 1/|legal|
// if sum <= 0), append the child block, back up the value along the path.
// per_copy: row rowbase[slot] + j holds copy j's result; else row = slot.

// An apply that cannot go on: the tree's status gets the error bit (its ctl is stored as the wave holds it) and
// the search's failure flag is raised; the host reports it at the move / search end
__device__ __forceinline__ void stop_tree(const Trees &tr, int t, TreeCtl &ctl, int32_t err_bit) {
    if (lane_id() != 0) return;
    ctl.status |= err_bit;
    tr.ctl[t] = ctl;
    flag_tree_error(tr);
}

__device__ __forceinline__ void apply_wave(Pool pool, Trees tr, EvalCache cache, const float *__restrict__ policy,
                                           int64_t pld, const float *__restrict__ value, int64_t vld,
                                           const int32_t *__restrict__ rowbase, int per_copy,
                                           unsigned long long *bytes_ctr, int slot, float *row /* LDS, 84 floats */,
                                           int by_tree = -1, int by_tree_depth = 0, float *copy_rows = nullptr,
                                           bool host_rows = false, CachePublish *defer = nullptr) {
    // copy_rows (LDS, 8 x 84 floats, 16-B aligned; optional): the per-copy prior sums of a chunk run in 8 lanes
    // at once instead of one copy after another. host_rows: the evaluation rows sit in fine-grained host
    // memory the host wrote behind a polled command; they are read with system-coherent (sc0 sc1) loads,
    // so no cache invalidation stands between the command and them (k_search1: one leaf, its rows from row 0,
    // at least 8 rows readable)
    auto ld_row = [host_rows](const float *a) -> float {
        return host_rows ? __hip_atomic_load(a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) : *a;
    };
    const int lane = lane_id();
    // two dependent round trips before the work: the count with this slot's tree and leaf depth
    // (tree_of / depth_of hold n_trees entries, stale past the count), then the tree's records, the
    // path entries 0..depth (round 4: all 128 were loaded, 2.5 KB a leaf) and the slot's evaluation.
    // by_tree >= 0 (one-dispatch hash rounds, k_round1): the tree and its leaf's depth are given and its
    // evaluation is row `slot` == by_tree (rows by tree, no scan)
    int t, dq;
    if (by_tree >= 0) {
        t = by_tree;
        dq = by_tree_depth;
    } else {
        const int cnt = tr.count[0];
        t = tr.tree_of[slot < tr.n_trees ? slot : 0];
        dq = tr.depth_of[slot < tr.n_trees ? slot : 0];
        if (slot >= cnt) return;
    }
    // host_rows, per copy: the first 8 rows (the host block holds at least 16) are loaded before the tree's
    // records, whose round trip they then share; masked by legality and by k once those have arrived
    constexpr int kCopyChunk = 8;
    float h0[kCopyChunk], h1[kCopyChunk], hv[kCopyChunk];
    if (host_rows && per_copy) {
#pragma unroll
        for (int jj = 0; jj < kCopyChunk; ++jj) {
            const float *pol = policy + (int64_t)jj * pld;
            h0[jj] = ld_row(pol + lane);
            h1[jj] = ld_row(pol + 64 + (lane < 17 ? lane : 16));
            hv[jj] = ld_row(value + (int64_t)jj * vld);
        }
    }
    const LeafRec r = tr.rec[t];
    TreeCtl ctl = tr.ctl[t];
    const uttt_state_t s = tr.leaf[t];
    const size_t base = (size_t)t * pool.cap;
    const int32_t *gp = tr.path + (size_t)t * kMaxDepth;
    const uint4 *gr = tr.path_rec + (size_t)t * kMaxDepth;
    int g_lo = 0, g_hi = 0;
    uint4 pr_lo = {0u, 0u, 0u, 0u}, pr_hi = {0u, 0u, 0u, 0u};  // the path nodes' records as the select read them
    if (lane <= dq) {
        g_lo = gp[lane];
        pr_lo = gr[lane];
    }
    if (lane + 64 <= dq) {
        g_hi = gp[lane + 64];
        pr_hi = gr[lane + 64];
    }
    float raw0 = 0.0f, raw1 = 0.0f, rawv = 0.0f;
    if (!per_copy) {
        const float *pol = policy + (int64_t)slot * pld;
        raw0 = ld_row(pol + lane);
        raw1 = ld_row(pol + 64 + (lane < 17 ? lane : 16));
        rawv = ld_row(value + (int64_t)slot * vld);
    }
    const int depth = r.depth;
    const int k = r.k;
    const int pn_lo = lane <= depth ? g_lo : 0;
    const int pn_hi = lane + 64 <= depth ? g_hi : 0;
    int L = 0;
    bool inserted = false;
    const int nodes_before = ctl.node_count;
    if (!per_copy) {
        const float v = rawv;
        // SURVEY §5 failure detection: a NaN / Inf legal prior or value (uttt_mcts.cpp:144-166 would
        // expand and back it up silently) stops the tree with kErrNonFinite, which the host raises at
        // the move boundary (UTTT_ERR_NONFINITE); nothing of it is expanded or cached. A non-finite
        // entry of an illegal action is never read by the search (it is expanded as the reference
        // would), but such a row is not cached either: the table only ever holds finite rows.
        const bool fin0 = __builtin_isfinite(raw0), fin1 = __builtin_isfinite(raw1);
        {
            uint32_t m[3];
            legal_mask(s, m);
            const bool bad = (bit_of(m, lane) && !fin0) || (lane < 17 && bit_of(m, 64 + lane) && !fin1) ||
                             !__builtin_isfinite(v);
            if (__ballot(bad)) {
                stop_tree(tr, t, ctl, kErrNonFinite);
                return;
            }
        }
        const bool cacheable = __ballot(!fin0 || (lane < 17 && !fin1)) == 0ull;
        // the insert's flag loads go out before the expansion's work, which runs under their round trip
        const CacheProbe ipr = cache_probe_issue(cache, s);
        float psum = 0.0f;
        if (!expand_backup(pool, base, r.node, depth, pn_lo, pn_hi, pr_lo, pr_hi, k, s, raw0, lane < 17 ? raw1 : 0.0f,
                           v, ctl.node_count, tr.py != 0, row, false, 0.0f, &psum)) {
            stop_tree(tr, t, ctl, kErrCapacity);
            return;
        }
        inserted = cacheable && cache_insert(cache, ipr, s, raw0, raw1, v, tr.py == 0, psum, defer);
        L = (ctl.node_count - nodes_before) / k;
    } else {
        // the reference's exact call pattern: k results, one per queued copy, applied in order
        const Legal g = legal_of(s);
        const bool l0 = g.l0, l1 = g.l1;
        const uint64_t b0 = g.b0, b1 = g.b1;
        const int i0 = g.i0, i1 = g.i1;
        L = g.L;
        const int nb = ctl.node_count;
        if ((int64_t)nb + (int64_t)k * L > pool.cap || L == 0) {
            stop_tree(tr, t, ctl, kErrCapacity);
            return;
        }
        // the copies' rows in chunks of kCopyChunk whose loads are all issued before the first use: one
        // memory round trip per chunk instead of one per copy (the rows of a one-tree search sit in host
        // memory, a PCIe round trip each: round 6 measured 16 us of a flush's apply on 8 sequential rows)
        const int64_t rb = rowbase[slot];
        float c0[kCopyChunk], c1[kCopyChunk], cv[kCopyChunk];
        auto load_chunk = [&](int j0) {
            if (host_rows && j0 == 0) {  // the prefetched rows (row base 0)
#pragma unroll
                for (int jj = 0; jj < kCopyChunk; ++jj) {
                    const int q = jj < k ? jj : 0;
                    float x0 = h0[0], x1 = h1[0], xv = hv[0];
#pragma unroll
                    for (int i = 1; i < kCopyChunk; ++i) {
                        x0 = q == i ? h0[i] : x0;
                        x1 = q == i ? h1[i] : x1;
                        xv = q == i ? hv[i] : xv;
                    }
                    c0[jj] = l0 ? x0 : 0.0f;
                    c1[jj] = l1 ? x1 : 0.0f;
                    cv[jj] = xv;
                }
                return;
            }
#pragma unroll
            for (int jj = 0; jj < kCopyChunk; ++jj) {
                const int64_t row = rb + (j0 + jj < k ? j0 + jj : j0);
                const float *pol = policy + row * pld;
                c0[jj] = l0 ? ld_row(pol + lane) : 0.0f;
                c1[jj] = l1 ? ld_row(pol + 64 + lane) : 0.0f;
                cv[jj] = ld_row(value + row * vld);
            }
        };
        // copy_rows: lane jj's sum of the chunk's copy jj, its legal priors compacted in action order into an
        // LDS row (seq_sum_legal's order and zero padding, so the same f32 sum as the one-lane loop below)
        float csum = 0.0f;
        auto chunk_sums = [&]() {
#pragma unroll
            for (int jj = 0; jj < kCopyChunk; ++jj) store_ranked_row(copy_rows + jj * 84, c0[jj], c1[jj], g);
            csum = sum_row4(copy_rows + (lane & (kCopyChunk - 1)) * 84, L);
        };
        bool bad = false;  // any copy's legal prior or value non-finite: nothing is applied (as above)
        for (int j0 = 0; j0 < k; j0 += kCopyChunk) {
            load_chunk(j0);
#pragma unroll
            for (int jj = 0; jj < kCopyChunk; ++jj)
                bad |= !__builtin_isfinite(c0[jj]) || !__builtin_isfinite(c1[jj]) || !__builtin_isfinite(cv[jj]);
        }
        if (__ballot(bad)) {
            stop_tree(tr, t, ctl, kErrNonFinite);
            return;
        }
        uint4 r_lo = pr_lo, r_hi = pr_hi;
        float w_lo = __uint_as_float(r_lo.x), w_hi = __uint_as_float(r_hi.x);
        for (int j = 0; j < k; ++j) {
            const int jj = j & (kCopyChunk - 1);
            if (jj == 0 && k > kCopyChunk) load_chunk(j);  // k <= kCopyChunk: the check's chunk is still held
            if (jj == 0 && copy_rows) chunk_sums();
            float p0 = c0[0], p1 = c1[0], v = cv[0];
#pragma unroll
            for (int i = 1; i < kCopyChunk; ++i) {
                p0 = jj == i ? c0[i] : p0;
                p1 = jj == i ? c1[i] : p1;
                v = jj == i ? cv[i] : v;
            }
            float sum = 0.0f;
            if (copy_rows) {
                sum = readlane_f(csum, jj);
            } else {
                for (uint64_t bits = b0; bits; bits &= bits - 1ull) sum += readlane_f(p0, __builtin_ctzll(bits));
                for (uint64_t bits = b1; bits; bits &= bits - 1ull) sum += readlane_f(p1, __builtin_ctzll(bits));
            }
            const float un = 1.0f / (float)L;
            const float q0 = sum > 0 ? p0 / sum : un;
            const float q1 = sum > 0 ? p1 / sum : un;
            const size_t blk = base + nb + (size_t)j * L;
            if (l0) pool.rec[blk + i0] = new_child(q0, (uint32_t)lane);
            if (l1) pool.rec[blk + i1] = new_child(q1, (uint32_t)(64 + lane));
            if (lane <= depth) w_lo += ((depth - lane) & 1) ? -v : v;
            if (lane + 64 <= depth) w_hi += ((depth - lane - 64) & 1) ? -v : v;
        }
        // path nodes: w, N += k; the leaf (depth) also gets L and its link (first child, k blocks)
        auto put = [&](uint4 rr, float w, int pn, int d) {
            rr.x = __float_as_uint(w);
            rr.z += (uint32_t)k;
            if (d == depth) {
                rr.z = (rr.z & ~kMetaLMask) | ((uint32_t)L << 23);
                rr.w = make_link((uint32_t)nb, (uint32_t)k);
            }
            pool.rec[base + pn] = rr;
        };
        if (lane <= depth) put(r_lo, w_lo, pn_lo, lane);
        if (lane + 64 <= depth) put(r_hi, w_hi, pn_hi, lane + 64);
        ctl.node_count = nb + k * L;
    }
    if (lane == 0) {
        ctl.sims_done += k;
        tr.ctl[t] = ctl;
        if (bytes_ctr) {
            // algorithmic bytes of one leaf: the slot's tree, depth and count (12), its LeafRec, TreeCtl and
            // state (64), the path's indices and records (20 per level), the evaluation (328 per copy);
            // written: the k child blocks (16 per child), the path's records (16 per level), the TreeCtl
            // (16); with the evaluation cache: the probe's 8 flags (32) and a new record (368 + 4)
            const int copies = per_copy ? k : 1;
            const unsigned long long b = 12ull + 64ull + 36ull * (unsigned long long)(depth + 1) + 328ull * copies +
                                         16ull * (unsigned long long)(k * L) + 16ull + (cache.flag ? 32ull : 0ull) +
                                         (inserted ? 372ull : 0ull);
            atomicAdd(stripe_of(bytes_ctr), b);
        }
    }
}

__global__ __launch_bounds__(kBlock) void k_apply(Pool pool, Trees tr, EvalCache cache, const float *__restrict__ policy,
                                                  int64_t pld, const float *__restrict__ value, int64_t vld,
                                                  const int32_t *__restrict__ rowbase, int per_copy,
                                                  unsigned long long *bytes_ctr) {
    __shared__ __attribute__((aligned(16))) float s_row[kWavesPerBlock][84];  // the prior sum's row, per wave
    apply_wave(pool, tr, cache, policy, pld, value, vld, rowbase, per_copy, bytes_ctr, wave_index(),
               s_row[threadIdx.x >> 6]);
}

// One flush of a one-tree search in one launch (round 5, uttt_search_select_host / _apply_host): the previous
// flush's evaluation applied (k_apply's body, reading it from pinned host memory), then the next descent
// (k_select's body), which stores the round's result to pinned host memory behind its tag. One wave, one
// dispatch per flush where k_apply, k_select and k_scan took three.
template <bool PY>
__global__ __launch_bounds__(kWave) void k_flush1(Pool pool, Trees tr, EvalCache cache, EvalCache apply_cache,
                                                  const float *__restrict__ policy, int64_t pld,
                                                  const float *__restrict__ value, int64_t vld,
                                                  const int32_t *__restrict__ rowbase, int per_copy, int do_apply,
                                                  unsigned long long *stats, HostLeaf *host_leaf, int32_t tag) {
    __shared__ __attribute__((aligned(16))) float s_row[84];
    if (do_apply) {
        apply_wave(pool, tr, apply_cache, policy, pld, value, vld, rowbase, per_copy,
                   stats ? stats + kKApply * kRow : nullptr, 0, s_row);
        wave_memory_fence();  // the descent reads the records the apply wrote
    }
    select_wave<PY>(pool, tr, cache, stats, 0, s_row, host_leaf, tag);
}

// The hash evaluator's outputs for one state into row `row` (k_hash_leaves' and k_round1's): bit j = ch * 81 +
// R * 9 + C of the network input, as k_encode writes it, so the words and outputs are k_hash_eval's.
// The network input of state s (m: its legal mask) as four ballot words over its 243 bits
__device__ __forceinline__ void input_words(const uttt_state_t &s, const uint32_t (&m)[3], uint64_t (&w)[4]) {
    const int lane = lane_id();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int j = i * 64 + lane;
        bool on = false;
        if (j < 243) {
            const int ch = j / 81, a = action_at(j % 81);
            on = (ch == 0 ? bit_of(s.own, a) : (ch == 1 ? bit_of(s.opp, a) : bit_of(m, a))) != 0u;
        }
        w[i] = __ballot(on);
    }
}
__device__ __forceinline__ void hash_leaf_row(const uttt_state_t &s, float *__restrict__ policy, float *__restrict__ value,
                                              int row) {
    const int lane = lane_id();
    uint32_t m[3];
    legal_mask(s, m);
    uint64_t w[4];
    input_words(s, m, w);
    const uint64_t h = hash_words(w);
    policy[(size_t)row * 81 + lane] = hash_prior(h, lane);
    if (lane < 17) policy[(size_t)row * 81 + 64 + lane] = hash_prior(h, 64 + lane);
    if (lane == 0) value[row] = hash_value(h);
}

// The select's slowest tree folded into the sums (as k_scan folds it): the max over the stripes of rows rm and
// rt, one stripe per lane l of one wave, which clears them
__device__ __forceinline__ void fold_select_max(unsigned long long *stats, int rm, int rt, int l) {
    unsigned long long ml = 0ull, mt = 0ull;
    if (l < kStripes) {
        unsigned long long *a = stats + rm * kRow + l * kStripeStride;
        unsigned long long *bb = stats + rt * kRow + l * kStripeStride;
        ml = __hip_atomic_load(a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        mt = __hip_atomic_load(bb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(a, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(bb, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long ol = __shfl_xor(ml, off), ot = __shfl_xor(mt, off);
        ml = ol > ml ? ol : ml;
        mt = ot > mt ? ot : mt;
    }
    if (l == 0) {
        stats[kKSelMaxSum * kRow] += ml;
        stats[kKSelTripMaxSum * kRow] += mt;
    }
}

// One tree-only round in ONE dispatch (round 6; UTTT_FUSED_ROUNDS=0 keeps the public calls'
// k_select + k_scan + k_hash_leaves + k_apply). With the hash evaluator nothing needs the leaves in slot order,
// so the rows are indexed by TREE: wave t applies its tree's evaluation of the previous round from row t
// (apply != 0 and its pending word, still the previous round's, shows a queued leaf), runs the next descent
// (k_select's body), and evaluates the leaf it queued straight into row t. The round's counts, which k_scan
// produces for the other rounds, are summed per block into a partial (sc1 store) and the last block to arrive
// (striped arrival counters, then one top counter) adds the partials, publishes them (device counts, the host
// ring and its tag) and resets the counters for the next round. Every tree's work is k_apply's and k_select's
// in the same order, so every result is the unfused round's (the fused-rounds test runs both).
constexpr int kR1Stripes = 8;
// uttt_rounds_hash_move's per-block count words: n0 (queued leaves) bits 0-4, n1 (budget stops) 5-9, n2
// (trees with simulations left) 10-14, at most kWavesPerBlock = 16 each; the round's tag (17 bits) above
constexpr int kPartTagShift = 15;
constexpr uint32_t kPartTagMask = 0x1FFFFu;
constexpr uint32_t kPartLiveMask = 0x1Fu | (0x1Fu << 10);
static_assert(kWavesPerBlock <= 31, "k_round1's per-block count words hold 5-bit counts");
constexpr int kR1Partial = 64;  // rctl: [0..7] stripe arrivals, [32] top, [64 + block] partials
template <bool PY>
__global__ __launch_bounds__(kBlock, 4) void k_round1(Pool pool, Trees tr, EvalCache cache, const float *apply_policy,
                                                   const float *apply_value, float *__restrict__ policy,
                                                   float *__restrict__ value, int apply, unsigned long long *stats,
                                                   int32_t *host_count, int32_t tag, uint32_t *rctl,
                                                   uint32_t *part_host, uint32_t *part_dev, const uint32_t *part_prev,
                                                   int nb_prev, int stats_parity) {
    __shared__ __attribute__((aligned(16))) float s_row[kWavesPerBlock][84];
    __shared__ uint32_t s_cnt;
    __shared__ int s_last;
    // part_host (uttt_rounds_hash_move's rounds, no kernel timing): no last-block publish. Each block stores its
    // counts with the round's tag into its own word of a host array (and of a device array the next round's
    // empty-round check reads, part_prev), and the host sums the words once every block's has the tag: the
    // arrival atomics, the partials' reload and the last block's drain left each round's critical path (round 6)
    if (part_host) {
        if (stats && blockIdx.x == 0 && threadIdx.x < kWave) {
            // the previous round's slowest tree (the other parity's rows) into the sums; this round's waves
            // write this parity's rows meanwhile
            fold_select_max(stats, stats_parity ? kKSelMax : kKSelMaxB, stats_parity ? kKSelTripMax : kKSelTripMaxB,
                            (int)threadIdx.x);
        }
        const uint32_t t17 = ((uint32_t)tag & kPartTagMask) << kPartTagShift;
        bool empty = false;
        if (part_prev) {  // the previous round queued no leaf and left no tree with simulations
            bool busy = false;
            for (int i = threadIdx.x; i < nb_prev; i += kBlock) busy |= (part_prev[i] & kPartLiveMask) != 0u;
            empty = !__syncthreads_or(busy);
        }
        if (empty) {
            if (threadIdx.x == 0) {
                part_dev[blockIdx.x] = t17;
                __hip_atomic_store(part_host + blockIdx.x, t17, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
            return;
        }
    }
    // a round behind one that queued no leaf and left no tree with simulations (the host's look-ahead rounds
    // past a move's end) has nothing to apply or select: every pending word is already 0 and the counts
    // stay 0, so block 0 publishes them and its tag, and every other block leaves at once (round 6: such a
    // round cost ~19 us of GPU time as a full pass over the trees; k_begin marks a new search non-empty)
    if (!part_host && tr.count[0] == 0 && tr.count[2] == 0) {
        if (blockIdx.x == 0 && threadIdx.x == 0 && host_count) {
            st_host(host_count + 0, 0);
            st_host(host_count + 1, 0);
            st_host(host_count + 2, 0);
            host_stores_done();
            st_host(host_count + 3, tag);
        }
        return;
    }
    const int t = wave_index();
    const int lane = lane_id();
    if (threadIdx.x == 0) s_cnt = 0u;
    __syncthreads();
    CachePublish held{-1, 0u};  // the apply's cache insert, published after this block's drain below
    if (t < tr.n_trees) {
        const int prev = __builtin_amdgcn_readfirstlane(tr.pending[t]);  // the previous round's, until the select
        if (apply && (prev & 1)) {
            apply_wave(pool, tr, cache, apply_policy, 81, apply_value, 1, nullptr, 0,
                       stats ? stats + kKApply * kRow : nullptr, t, s_row[threadIdx.x >> 6], t, prev >> 8, nullptr,
                       false, &held);
            wave_memory_fence();  // the descent reads the records the apply wrote
        }
        uttt_state_t leaf;
        const int p = select_wave<PY>(pool, tr, cache, stats, t, s_row[threadIdx.x >> 6], nullptr, 0,
                                      part_host ? stats_parity : 0, &leaf);
        if (p & 1) hash_leaf_row(leaf, policy, value, t);  // the queued leaf (its state from the descent)
        const int q = p & 0xFF;
        if (lane == 0)  // pending | stopped << 10 | left << 20 (at most kWavesPerBlock each)
            atomicAdd(&s_cnt, (uint32_t)((q == 1 || q == 3) ? 1 : 0) | ((q == 2 ? 1u : 0u) << 10) |
                                  ((q >= 2 ? 1u : 0u) << 20));
    }
    // every wave's stores (rows, records, stats atomics, a held cache record) complete before the block's
    // partial is published, and before the held record's flag
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    cache_publish(cache, held);
    __syncthreads();
    if (part_host) {  // the block's counts and the round's tag, one word (its stores drained above)
        if (threadIdx.x == 0) {
            const uint32_t w = (((uint32_t)tag & kPartTagMask) << kPartTagShift) | ((s_cnt >> 20) << 10) |
                               (((s_cnt >> 10) & 0x3FFu) << 5) | (s_cnt & 0x3FFu);
            part_dev[blockIdx.x] = w;
            __hip_atomic_store(part_host + blockIdx.x, w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        return;
    }
    const int nb = (int)gridDim.x, b = (int)blockIdx.x;
    if (threadIdx.x == 0) {
        __hip_atomic_store(rctl + kR1Partial + b, s_cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const int st = b & (kR1Stripes - 1);
        const uint32_t in_stripe = (uint32_t)((nb - st + kR1Stripes - 1) / kR1Stripes);
        const int stripes = nb < kR1Stripes ? nb : kR1Stripes;
        int last = 0;
        if (__hip_atomic_fetch_add(rctl + st, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == in_stripe - 1)
            last = __hip_atomic_fetch_add(rctl + 32, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ==
                   (uint32_t)(stripes - 1);
        s_last = last;
    }
    __syncthreads();
    if (!s_last) return;
    // the last block: every partial was published before its block's arrival (sc1 loads, no stale L1 copy)
    uint32_t c0 = 0u, c1 = 0u, c2 = 0u;
    for (int i = threadIdx.x; i < nb; i += kBlock) {
        const uint32_t v = __hip_atomic_load(rctl + kR1Partial + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        c0 += v & 0x3FFu;
        c1 += (v >> 10) & 0x3FFu;
        c2 += v >> 20;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        c0 += __shfl_xor(c0, off);
        c1 += __shfl_xor(c1, off);
        c2 += __shfl_xor(c2, off);
    }
    __shared__ uint32_t s_sum[3][kWavesPerBlock];
    if (lane == 0) {
        s_sum[0][threadIdx.x >> 6] = c0;
        s_sum[1][threadIdx.x >> 6] = c1;
        s_sum[2][threadIdx.x >> 6] = c2;
    }
    // the select's slowest tree (as k_scan folds it): the max over the stripes, one per lane of wave 1
    if (stats && threadIdx.x >= kWave && threadIdx.x < 2 * kWave)
        fold_select_max(stats, kKSelMax, kKSelTripMax, (int)threadIdx.x - kWave);
    __syncthreads();
    if (threadIdx.x == 0) {
        int n0 = 0, n1 = 0, n2 = 0;
        for (int w = 0; w < kWavesPerBlock; ++w) {
            n0 += (int)s_sum[0][w];
            n1 += (int)s_sum[1][w];
            n2 += (int)s_sum[2][w];
        }
        tr.count[0] = n0;
        tr.count[1] = n1;
        tr.count[2] = n2;
        for (int i = 0; i < kR1Stripes; ++i) rctl[i] = 0u;
        rctl[32] = 0u;
        if (host_count) {
            __hip_atomic_store(host_count + 0, n0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(host_count + 1, n1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(host_count + 2, n2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            host_stores_done();
            st_host(host_count + 3, tag);
        }
    }
}

// A one-dispatch round's staged evaluation applied by tree (flush before anything else reads the trees)
__global__ __launch_bounds__(kBlock) void k_apply_tree(Pool pool, Trees tr, EvalCache cache, const float *policy,
                                                       const float *value, unsigned long long *bytes_ctr) {
    __shared__ __attribute__((aligned(16))) float s_row[kWavesPerBlock][84];
    const int t = wave_index();
    if (t >= tr.n_trees) return;
    const int prev = __builtin_amdgcn_readfirstlane(tr.pending[t]);
    if (prev & 1)
        apply_wave(pool, tr, cache, policy, 81, value, 1, nullptr, 0, bytes_ctr, t, s_row[threadIdx.x >> 6], t,
                   prev >> 8);
}

// -------------------------------------------------------------- hash eval --
// Deterministic test evaluator on the NCHW rows: one wave per row; the 4
// ballots of "x != 0" over the 243 floats are exactly the 4 hash words.
__global__ __launch_bounds__(kBlock) void k_hash_eval(const float *__restrict__ x, int n, float *__restrict__ policy,
                                                      float *__restrict__ value) {
    const int lane = lane_id();
    const int row = wave_index();
    if (row >= n) return;
    const float *xr = x + (size_t)row * 243;
    uint64_t w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int j = i * 64 + lane;
        w[i] = __ballot(j < 243 && xr[j] != 0.0f);
    }
    const uint64_t h = hash_words(w);
    policy[(size_t)row * 81 + lane] = hash_prior(h, lane);
    if (lane < 17) policy[(size_t)row * 81 + 64 + lane] = hash_prior(h, 64 + lane);
    if (lane == 0) value[row] = hash_value(h);
}

// ---------------------------------------------------------- root results --
__device__ __forceinline__ int root_children(const Pool &pool, size_t base, int &first) {
    const uint4 r = pool.rec[base];
    first = link_first(r.w);
    return meta_L(r.z);
}
__device__ __forceinline__ int visits_of(const Pool &pool, size_t i) { return meta_n(pool.rec[i].z); }

// pv_mcts_scores' return value (uttt_mcts.cpp:177-195): root child visits as
// f32 -> one-hot first max (t == 0) or boltzman (:199-216).
__device__ void root_scores(const Pool &pool, size_t base, float temperature, float *sc, int &L) {
    int first;
    L = root_children(pool, base, first);
    if (temperature == 0.0f) {
        int mi = 0;
        float mv = L ? (float)visits_of(pool, base + first) : 0.0f;
        for (int i = 1; i < L; ++i) {
            const float v = (float)visits_of(pool, base + first + i);
            if (v > mv) {
                mv = v;
                mi = i;
            }
        }
        for (int i = 0; i < L; ++i) sc[i] = (i == mi) ? 1.0f : 0.0f;
    } else {
        // glibc's powf (what the reference's std::pow(float, float) calls) evaluates in
        // double and rounds once; ocml's f32 powf is not correctly rounded (pow(19, 1)
        // came out 1 ulp low), so do the same: double pow of the f32 operands, one rounding.
        const double y = (double)(1.0f / temperature);
        float sum = 0.0f;
        for (int i = 0; i < L; ++i) {
            sc[i] = (float)pow((double)visits_of(pool, base + first + i), y);
            sum += sc[i];
        }
        if (sum > 0)
            for (int i = 0; i < L; ++i) sc[i] /= sum;
    }
}

// The same evaluator on this round's pending leaves straight from their states (the device-count
// rounds: no NCHW input is written): bit j = ch * 81 + R * 9 + C of the network input, as k_encode
// writes it, so the words and outputs are k_hash_eval's. One wave per slot; the count is read on the
// device (the grid covers every tree).
__global__ __launch_bounds__(kBlock) void k_hash_leaves(Trees tr, float *__restrict__ policy,
                                                        float *__restrict__ value) {
    const int row = wave_index();
    if (row >= tr.count[0]) return;
    const uttt_state_t s = tr.leaf[tr.tree_of[row]];
    hash_leaf_row(s, policy, value, row);
}

// ---------------------------------------------------------------- playouts --
// Random-playout evaluator (uttt_playout.h; game.py:277-287 `playout`, the evaluation of game.py:294-379's
// mcts_action): one wave per position, lane = playout, ceil(P / 64) passes. The position is wave-uniform; each
// lane plays its own game on a private copy of the 32-byte state in registers until it ends (at most 81 plies;
// the wave leaves the loop with its last lane), and a pass's wins and losses are two ballots' popcounts.
// No LDS, no atomics, no scratch.
__device__ __forceinline__ void playout_wave(const uttt_state_t &s, int P, uint64_t seed, int32_t &wins, int32_t &losses) {
    const int lane = lane_id();
    uint32_t m[3];
    legal_mask(s, m);
    uint64_t w[4];
    input_words(s, m, w);
    const uint64_t h = playout_key(w, seed);
    wins = losses = 0;
    for (int base = 0; base < P; base += kWave) {
        const int j = base + lane;
        int r = 0;
        if (j < P) r = playout(s, h, (uint32_t)j);
        wins += (int32_t)__popcll(__ballot(r > 0));
        losses += (int32_t)__popcll(__ballot(r < 0));
    }
}

// The round's evaluator, shaped like k_hash_leaves (one wave per slot, the count read on the device): the
// value is the mean playout result; the priors are 81 x 1, which k_apply's legal mask and sequential
// renormalisation turn into exactly 1 / |legal|.
__global__ __launch_bounds__(kBlock) void k_playout_leaves(Trees tr, int P, uint64_t seed, float *__restrict__ policy,
                                                           float *__restrict__ value) {
    const int row = wave_index();
    if (row >= tr.count[0]) return;
    const int lane = lane_id();
    const uttt_state_t s = tr.leaf[tr.tree_of[row]];
    int32_t wins, losses;
    playout_wave(s, P, seed, wins, losses);
    policy[(size_t)row * 81 + lane] = 1.0f;
    if (lane < 17) policy[(size_t)row * 81 + 64 + lane] = 1.0f;
    if (lane == 0) value[row] = playout_value(wins - losses, P);
}

// Flat Monte-Carlo on arbitrary positions, terminal ones included (a lost position: every playout a loss;
// a drawn one: neither): wins and losses of the side to move over P playouts, one wave per position.
__global__ __launch_bounds__(kBlock) void k_playout_states(const uttt_state_t *__restrict__ states, int n, int P,
                                                           uint64_t seed, int32_t *__restrict__ wins,
                                                           int32_t *__restrict__ losses) {
    const int row = wave_index();
    if (row >= n) return;
    const uttt_state_t s = states[row];
    int32_t nw, nl;
    playout_wave(s, P, seed, nw, nl);
    if (lane_id() == 0) {
        wins[row] = nw;
        losses[row] = nl;
    }
}

// ------------------------------------------------------------------ solver --
// Exact endgame values (uttt_solve.h; game.py:240-274 `alpha_beta` / `alpha_beta_action`): one wave per
// position, lane i searches the child of the i-th legal action. The position is wave-uniform; each lane keeps
// the node it is at in registers and its frames in LDS, frame d of lane l at word d * 64 + l of the wave's
// block: whatever depths the lanes are at, lane l reads and writes bank l % 64 only, so no step has a bank
// conflict (lane-contiguous stacks of 32 words put every second lane at one depth on one bank). One trip of the loop is
// one step of the machine for every live lane; the wave leaves with its last lane. No atomics, no scratch;
// each wave writes its own position's outputs only.
struct LdsStack {
    uint32_t *base;  // this lane's frame 0
    __device__ __forceinline__ uint32_t load(int d) const { return base[d * kWave]; }
    __device__ __forceinline__ void store(int d, uint32_t x) { base[d * kWave] = x; }
};
static_assert(sizeof(uint32_t) * kWavesPerBlock * kSolveMaxEmpty * kWave <= 65536,
              "k_solve_states, k_solve_leaves: LDS per workgroup");

__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off));
    return v;
}
__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// Legal actions below action j: the lane that searched j, when j is legal.
__device__ __forceinline__ int legal_rank(const uint32_t m[3], int j) {
    int r = 0;
#pragma unroll
    for (int w = 0; w < 3; ++w) {
        const int k = j - 27 * w;
        r += (int)popc32(k <= 0 ? 0u : (k >= 27 ? m[w] : m[w] & ((1u << k) - 1u)));
    }
    return r;
}

// The machine both solver kernels run on a searched position (solve_root said so): lane i < L searches the
// child of the i-th legal move on this wave's block of `frames`. av: this lane's action value
// (UTTT_SOLVE_UNKNOWN for a lane without a move or out of budget); total: the nodes of all lanes; best / every:
// solve_result's arguments. All but av are wave-uniform.
__device__ __forceinline__ void solve_wave(const uttt_state_t &s, const uint32_t m[3], int32_t max_nodes,
                                           uint32_t *frames, int &av, int &total, int &best, bool &every) {
    const int lane = lane_id();
    const int L = (int)(popc32(m[0]) + popc32(m[1]) + popc32(m[2]));  // <= empties(s) <= 64
    const bool mine = lane < L;
    SolveLane ln;
    solve_lane_begin(ln, next_state(s, mine ? nth_legal(m, (uint32_t)lane) : 0));
    ln.live = mine;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    LdsStack stack{frames + wave * (kSolveMaxEmpty * kWave) + lane};
    while (__ballot(ln.live != 0) != 0ull) {
        if (ln.live) solve_step(ln, stack, max_nodes);
    }
    const bool known = mine && ln.solved;
    av = known ? -ln.v : UTTT_SOLVE_UNKNOWN;
    total = wave_sum_i(mine ? ln.nodes : 0);  // <= 64 * 2^22
    best = wave_max_i(known ? av : -2);
    every = __ballot(mine && !ln.solved) == 0ull;
}

// The values of actions `lane` and 64 + lane (the latter for lane < 17) from the lanes that searched them:
// action j's value sits in lane legal_rank(j). Meaningful for legal actions only.
__device__ __forceinline__ void action_values_of(const uint32_t m[3], int av, int &v0, int &v1) {
    const int lane = lane_id(), j1 = 64 + lane;
    v0 = __shfl(av, legal_rank(m, lane) & (kWave - 1));
    v1 = __shfl(av, legal_rank(m, j1 < 81 ? j1 : 80) & (kWave - 1));
}

__global__ __launch_bounds__(kBlock) void k_solve_states(const uttt_state_t *__restrict__ states, int n,
                                                         int32_t max_nodes, int8_t *__restrict__ value,
                                                         int8_t *__restrict__ action, int8_t *__restrict__ status,
                                                         int64_t *__restrict__ nodes,
                                                         int8_t *__restrict__ action_values) {
    __shared__ uint32_t frames[kWavesPerBlock * kSolveMaxEmpty * kWave];
    const int row = wave_index();
    if (row >= n) return;
    const int lane = lane_id();
    const uttt_state_t s = states[row];
    uint32_t m[3];
    legal_mask(s, m);
    int8_t st, val;
    int act = -1, total = 0;
    int av = UTTT_SOLVE_UNKNOWN;  // this lane's action value
    if (!solve_root(s, m, st, val)) {
        int best;
        bool every;
        solve_wave(s, m, max_nodes, frames, av, total, best, every);
        if (solve_result(best, every, st, val))  // the lowest move that reaches the value (unknown lanes: -128)
            act = nth_legal(m, (uint32_t)(__ffsll((long long)__ballot(av == best)) - 1));
    }
    const int j1 = 64 + lane;
    int v0, v1;
    action_values_of(m, av, v0, v1);
    int8_t *out = action_values + (size_t)row * 81;
    out[lane] = (int8_t)(bit_of(m, lane) ? v0 : UTTT_SOLVE_UNKNOWN);
    if (j1 < 81) out[j1] = (int8_t)(bit_of(m, j1) ? v1 : UTTT_SOLVE_UNKNOWN);
    if (lane == 0) {
        value[row] = val;
        action[row] = (int8_t)act;
        status[row] = st;
        nodes[row] = (int64_t)total;
    }
}

// The overlay of uttt_solve.h on the round's pending leaves, shaped like k_playout_leaves (one wave per slot,
// the count read on the device) and run after an evaluator has filled the rows: a leaf with more than
// max_empties empties leaves at once (the test is wave-uniform: in the opening the kernel costs its launch
// and one state load per leaf); the others run k_solve_states' machine, and a SOLVED one overwrites its
// row's value and, with UTTT_PRIORS_OPTIMAL, its 81 priors. The same 32 KB of LDS per workgroup, no
// scratch, no atomics; each wave writes its own row only.
__global__ __launch_bounds__(kBlock) void k_solve_leaves(Trees tr, int32_t max_empties, int32_t max_nodes,
                                                         int32_t priors, float *__restrict__ policy,
                                                         int64_t policy_ld, float *__restrict__ value,
                                                         int64_t value_ld, int8_t *__restrict__ status) {
    __shared__ uint32_t frames[kWavesPerBlock * kSolveMaxEmpty * kWave];
    const int row = wave_index();
    if (row >= tr.count[0]) return;
    const int lane = lane_id();
    const uttt_state_t s = tr.leaf[tr.tree_of[row]];
    int8_t st = UTTT_OVERLAY_SKIPPED, val = 0;
    bool searched = false;
    int av = UTTT_SOLVE_UNKNOWN;
    uint32_t m[3] = {0u, 0u, 0u};
    if (!overlay_skips(s, max_empties)) {
        legal_mask(s, m);
        searched = !solve_root(s, m, st, val);
        if (searched) {
            int total, best;
            bool every;
            solve_wave(s, m, max_nodes, frames, av, total, best, every);
            solve_result(best, every, st, val);
        }
    }
    if (status && lane == 0) status[row] = st;
    if (st != UTTT_SOLVE_SOLVED) return;
    if (lane == 0) value[(size_t)row * value_ld] = (float)val;
    if (!searched || priors != UTTT_PRIORS_OPTIMAL) return;
    const int j1 = 64 + lane;
    int v0, v1;
    action_values_of(m, av, v0, v1);
    float *out = policy + (size_t)row * policy_ld;
    out[lane] = overlay_prior(bit_of(m, lane) != 0u, v0, val);
    if (j1 < 81) out[j1] = overlay_prior(bit_of(m, j1) != 0u, v1, val);
}

__global__ void k_root_visits(Pool pool, Trees tr, int32_t *visits, int32_t *n_legal) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= tr.n_trees * 81) return;
    const int t = g / 81, i = g % 81;
    const size_t base = (size_t)t * pool.cap;
    int first;
    const int L = root_children(pool, base, first);
    visits[g] = i < L ? visits_of(pool, base + first + i) : 0;
    if (i == 0) n_legal[t] = L;
}

__global__ void k_root_scores(Pool pool, Trees tr, float temperature, float *scores, int32_t *n_legal) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= tr.n_trees) return;
    float *sc = scores + (size_t)t * 81;  // the output row is the working buffer (no scratch)
    int L;
    root_scores(pool, (size_t)t * pool.cap, temperature, sc, L);
    for (int i = L; i < 81; ++i) sc[i] = 0.0f;
    n_legal[t] = L;
}

// ------------------------------------------------- resident one-tree search --
// A whole one-tree search as ONE resident wave (round 6; uttt_search1_*): the reference's
// pv_mcts_scores (uttt_mcts.cpp:84-196) driven through python_bindings.cpp:11-47 calls the model once per
// flush, so the search needs the host between flushes; instead of a launch per flush (k_flush1), the wave
// stays resident and meets the host through fine-grained pinned memory (Search1Host): it writes the flush's
// leaf, its copies and a sequence tag (system-scope release), polls for the host's command (the evaluation
// rows the host wrote beside it, then the command's sequence), applies them (k_apply's body) and descends
// to the next leaf (k_select's body); when the tree has no simulation left it computes the root's scores
// (k_root_scores' body) into host memory and exits. Same tree, same order of operations as k_begin +
// k_flush1 + k_root_scores, so the same results. Exit conditions every path reaches: the search's end, the
// host's exit word, and 100 ms without a command (s_memrealtime at 100 MHz); after a timeout the host
// relaunches the wave in resume mode (the command it wrote is applied first).
struct Search1Host {
    // device -> host
    int32_t tag, count, k, status;  // a leaf (count 1) or the end (count 0); status: the tree's error bits
    int32_t n_legal, gone, pad0, pad1;  // gone: the command sequence the wave timed out waiting for (0: none)
    // the wave's time split (s_memrealtime ticks of 10 ns, this launch): descents, applies, waits for the host
    int32_t t_select, t_apply, t_wait, pad3;
    uttt_state_t leaf;
    float scores[84];  // 81 used
    // host -> device: the command, sequence (low word) and rows (high word) in one 8-byte store the wave
    // reads whole; the exit word
    uint64_t cmd;
    int32_t cmd_exit, pad2;
    // the evaluation rows: policy [rows][96] (81 used), value [rows] (one leaf: its row base is 0)
};
static_assert(offsetof(Search1Host, cmd) % 8 == 0, "Search1Host::cmd must be 8-byte aligned");

constexpr int kSearch1Timeout = 10000000;  // 100 ms of s_memrealtime (100 MHz)

template <bool PY>
__global__ __launch_bounds__(kWave) void k_search1(Pool pool, Trees tr, EvalCache cache, uttt_state_t root,
                                                   float temperature, Search1Host *hs, const float *policy,
                                                   const float *value, int32_t seq, int32_t resume) {
    __shared__ __attribute__((aligned(16))) float s_row[84];
    __shared__ int32_t s_rowbase;  // the flush's first row: 0 (in LDS, not a PCIe round trip per apply)
    __shared__ __attribute__((aligned(16))) float s_copies[8 * 84];  // per-copy rows' prior sums (apply_wave)
    const int lane = lane_id();
    if (lane == 0) s_rowbase = 0;
    if (!resume) {  // as k_begin for tree 0
        init_root(pool, tr, 0, root, true, tr.py);
        wave_memory_fence();
    }
    bool apply = resume != 0;  // resume: the command of sequence `seq` is waiting in host memory
    int rows = resume ? (int)__builtin_amdgcn_readfirstlane((int)(
                            __hip_atomic_load(&hs->cmd, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) >> 32))
                      : 0;
    uint64_t tk_sel = 0, tk_apply = 0, tk_wait = 0, tk = __builtin_amdgcn_s_memrealtime();
    for (;;) {
        if (apply) {
            // per-copy rows bypass the evaluation cache (as host_apply_args)
            EvalCache acache = cache;
            if (rows > 1) acache.flag = nullptr;
            apply_wave(pool, tr, acache, policy, 96, value, 1, &s_rowbase, rows > 1 ? 1 : 0, nullptr, 0, s_row, 0,
                       __builtin_amdgcn_readfirstlane(tr.pending[0]) >> 8, s_copies, true);
            wave_memory_fence();  // the descent reads the records the apply wrote
            const uint64_t t1 = __builtin_amdgcn_s_memrealtime();
            tk_apply += t1 - tk;
            tk = t1;
        }
        const int p = select_wave<PY>(pool, tr, cache, nullptr, 0, s_row, nullptr, 0);
        const int q = p & 0xFF;
        {
            const uint64_t t1 = __builtin_amdgcn_s_memrealtime();
            tk_sel += t1 - tk;
            tk = t1;
        }
        if (q == 2) {  // stopped by the select budget before a leaf: descend again (as uttt_search_select_host)
            apply = false;
            continue;
        }
        ++seq;
        if (q == 1 || q == 3) {  // a leaf: hand it to the host
            wave_memory_fence();
            // the leaf (lanes 0-7, one store), its copies, the count and the time split, then the tag
            const int32_t lw = reinterpret_cast<const int32_t *>(&tr.leaf[0])[lane & 7];
            if (lane < 8) st_host(reinterpret_cast<int32_t *>(&hs->leaf) + lane, lw);
            if (lane == 0) {
                st_host(&hs->k, tr.rec[0].k);
                st_host(&hs->t_select, (int32_t)tk_sel);
                st_host(&hs->t_apply, (int32_t)tk_apply);
                st_host(&hs->t_wait, (int32_t)tk_wait);
                st_host(&hs->count, 1);
            }
            host_stores_done();
            if (lane == 0) st_host(&hs->tag, seq);
            // wait for the host's command of this sequence (its rows were written before it; they are read
            // with system-coherent loads, so the poll needs no acquire and its cache invalidation)
            const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
            int got = 0;
            for (;;) {
                uint64_t c = 0;
                int x = 0;
                if (lane == 0) {
                    c = __hip_atomic_load(&hs->cmd, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    x = __hip_atomic_load(&hs->cmd_exit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                }
                const int cs = __builtin_amdgcn_readfirstlane((int)(uint32_t)c);
                x = __builtin_amdgcn_readfirstlane(x);
                if (cs == seq) {
                    rows = __builtin_amdgcn_readfirstlane((int)(c >> 32));
                    got = 1;
                    break;
                }
                if (x) break;
                if (__builtin_amdgcn_s_memrealtime() - t0 > (uint64_t)kSearch1Timeout) {
                    if (lane == 0) st_host(&hs->gone, seq);
                    host_stores_done();
                    break;
                }
                __builtin_amdgcn_s_sleep(1);
            }
            if (!got) return;
            const uint64_t t1 = __builtin_amdgcn_s_memrealtime();
            tk_wait += t1 - tk;
            tk = t1;
            apply = true;
            continue;
        }
        // the search's end: the root's scores (k_root_scores' body) and the tree's status, then the tag
        wave_memory_fence();
        int L = 0;
        if (lane == 0) root_scores(pool, 0, temperature, s_row, L);  // the LDS row as the working buffer
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        L = __builtin_amdgcn_readfirstlane(L);
        for (int i = lane; i < 81; i += kWave) st_host(&hs->scores[i], i < L ? s_row[i] : 0.0f);
        if (lane == 0) {
            st_host(&hs->n_legal, L);
            st_host(&hs->t_select, (int32_t)tk_sel);
            st_host(&hs->t_apply, (int32_t)tk_apply);
            st_host(&hs->t_wait, (int32_t)tk_wait);
            st_host(&hs->status, (int32_t)(tr.ctl[0].status & kErrMask));
            st_host(&hs->count, 0);
        }
        host_stores_done();
        if (lane == 0) st_host(&hs->tag, seq);
        return;
    }
}

// -------------------------------------------------------------- self-play --
struct Slot {
    uttt_state_t state;
    int64_t game;        // game id being played (-1: none)
    int32_t ply;
    int32_t live;
    int32_t finished;    // set by k_move_end when the game just ended
    int32_t fin_len;
    int64_t fin_game;
    int64_t fin_offset;  // arena row of its first ply
    int32_t fin_value;   // value of ply 0 (self_play_cpp.py:95)
    int32_t seed_pending;  // 1: k_finalize gave the slot a new game whose MT19937 key k_archive seeds
};

static_assert(offsetof(Slot, ply) == 40 && offsetof(Slot, live) == 44 && offsetof(Slot, finished) == 48 &&
                  offsetof(Slot, fin_len) == 52,
              "k_finalize reads Slot bytes 40..55 as one int4 (ply, live, finished, fin_len)");

struct GameEntry {
    int64_t game;
    int64_t offset;
    int64_t length;
};

struct SelfPlay {
    Slot *slot;
    uint32_t *mt_key;      // [slot][624]
    int32_t *mt_pos;       // [slot]
    uttt_state_t *ply_state;  // [slot][81]
    double *ply_policy;    // [slot][81][81]
    int8_t *ply_action;    // [slot][81]
    uttt_state_t *ar_state;
    double *ar_policy;
    int8_t *ar_action;
    int8_t *ar_value;
    GameEntry *games;
    int64_t *ctr;          // [0] next game id, [1] games finished, [2] arena plies used
    int32_t *live;         // [slot] flags for k_begin
    int32_t *work;         // [1 + slot]: k_finalize's count, then the slots k_archive has work for
    int64_t game_end;
    int64_t arena_cap;
    int64_t games_cap;
    uint32_t seed_base;
    float temperature;
    int32_t slots;
    // the temperature schedule (uttt_selfplay_set_temperature_schedule): `temperature` while Slot.ply < temp_plies,
    // late_temperature from then on; INT32_MAX: one temperature for the whole game
    int32_t temp_plies = INT32_MAX;
    float late_temperature = 0.0f;
};

// numpy legacy RandomState: init_genrand(seed) (mt19937_seed), genrand_int32
// with the standard twist/tempering, random_sample = 53-bit double of 2 draws.
__device__ __forceinline__ uint32_t mt_temper(uint32_t y) {
    y ^= y >> 11;
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= y >> 18;
    return y;
}

// The standard twist of one 624-word key by the 64 lanes of a wave. Element i reads key[i], key[i + 1]
// (old; key[0] new for i = 623) and key[(i + 397) % 624] (old for i < 227, new beyond), so three
// stages, [0, 227), [227, 454), [454, 624), each lane loading all its inputs before any store, run the
// sequential loop's exact updates (a thread's 624 dependent round trips took most of k_move_end).
__device__ void mt_twist_wave(uint32_t *key) {
    const int lane = lane_id();
    constexpr int lo[3] = {0, 227, 454}, hi[3] = {227, 454, 624};
#pragma unroll
    for (int st = 0; st < 3; ++st) {
        uint32_t a[4], b[4], c[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = lo[st] + lane + 64 * j;
            if (i < hi[st]) {
                a[j] = key[i];
                b[j] = key[i + 1 < 624 ? i + 1 : 0];
                c[j] = key[i + 397 < 624 ? i + 397 : i + 397 - 624];
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = lo[st] + lane + 64 * j;
            if (i < hi[st]) {
                const uint32_t y = (a[j] & 0x80000000u) | (b[j] & 0x7fffffffu);
                uint32_t v = c[j] ^ (y >> 1);
                if (y & 1u) v ^= 0x9908b0dfu;
                key[i] = v;
            }
        }
        wave_memory_fence();  // this stage's words before the next stage reads them (other lanes)
    }
}

// np.add.reduce on a contiguous float64 vector (pairwise, 8 accumulators, blocks <= 128).
__device__ double np_sum(const double *a, int n, int stride) {
    if (n < 8) {
        double r = 0.0;
        for (int i = 0; i < n; ++i) r += a[i * stride];
        return r;
    }
    double r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = a[j * stride];
    int i = 8;
    for (; i < n - (n % 8); i += 8)
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] += a[(i + j) * stride];
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += a[i * stride];
    return res;  // n <= 81 < 128: a single pairwise block
}

// A float held by lane i of the wave (i uniform), to every lane.
__device__ __forceinline__ float lane_float(float x, int i) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), i));
}

// One wave per slot: the per-move tail of self_play_cpp.play (:63-92). Entry i of the root's score
// row lives in lane i (x0) and lane i - 64 (x1); what is order-free (the arg-max, the f32 sum of
// integer visit counts) is a wave reduction, what is not (np.sum's pairwise blocks, the cumsum of
// np.random.choice) runs the reference's additions in its order on the wave's LDS copy of the row, the
// same in every lane (round 5: on v_readlane operands; round 3's thread-per-slot form walked the row in
// LDS, 81-step dependent chains per pass with one wave per 64 slots).
// fail (the asynchronous form: the search's failure flag, Trees::count[3]): on a failure this move's end
// changes nothing (no draw, no record, no refill), as the blocking form refuses before it runs
__global__ __launch_bounds__(kBlock) void k_move_end(Pool pool, SelfPlay sp, const int32_t *fail) {
    const int lane = lane_id();
    const int s = wave_index();
    if (s >= sp.slots) return;
    // the loads that do not depend on each other are issued together (round 6: the failure word, the slot,
    // the key position and the root's record were four dependent round trips before the first draw)
    const size_t base = (size_t)s * pool.cap;
    const int32_t failed = fail ? *fail : 0;
    Slot sl = sp.slot[s];
    int32_t pos = sp.mt_pos[s];
    int first;
    const int L = root_children(pool, base, first);
    if (failed) return;
    sl.finished = 0;
    if (!sl.live) {
        if (lane == 0) sp.slot[s] = sl;
        return;
    }
    // np.random.choice's random_sample (numpy legacy: two 32-bit draws, 53-bit double); a key that
    // runs out is twisted by the wave (mt_twist_wave)
    uint32_t *key = sp.mt_key + (size_t)s * 624;
    const bool h0 = lane < L, h1 = lane + 64 < L;
    const int n0 = h0 ? visits_of(pool, base + first + lane) : 0;
    const int n1 = h1 ? visits_of(pool, base + first + lane + 64) : 0;
    uint32_t w1, w2;
    if (pos >= 623) {
        const uint32_t k623 = key[623];
        mt_twist_wave(key);
        if (pos == 623) {  // the first word was key[623] before the twist
            w1 = mt_temper(k623);
            w2 = mt_temper(key[0]);
            pos = 1;
        } else {
            w1 = mt_temper(key[0]);
            w2 = mt_temper(key[1]);
            pos = 2;
        }
    } else {
        w1 = mt_temper(key[pos]);
        w2 = mt_temper(key[pos + 1]);
        pos += 2;
    }
    const double u = ((double)(w1 >> 5) * 67108864.0 + (double)(w2 >> 6)) / 9007199254740992.0;
    const int ply = sl.ply;
    const float temperature = ply < sp.temp_plies ? sp.temperature : sp.late_temperature;  // (wave-uniform)
    // root visit counts (uttt_mcts.cpp:177-192, as root_scores): entry i in lane i / i - 64 (loaded above)
    double x0, x1;
    if (temperature == 0.0f) {
        // one-hot first max: the largest count, then the lowest index holding it (counts < 2^24, so
        // the f32 compares of the reference order them as the integers do)
        int kk = max(h0 ? (n0 << 8) | (255 - lane) : -1, h1 ? (n1 << 8) | (255 - 64 - lane) : -1);
#pragma unroll
        for (int o = 32; o; o >>= 1) kk = max(kk, __shfl_xor(kk, o));
        const int mi = kk < 0 ? 0 : 255 - (kk & 0xFF);
        x0 = (h0 && lane == mi) ? 1.0 : 0.0;
        x1 = (h1 && lane + 64 == mi) ? 1.0 : 0.0;
    } else {
        const double y = (double)(1.0f / temperature);  // glibc powf: double pow, one rounding
        float v0 = 0.0f, v1 = 0.0f, sum = 0.0f;
        if (y == 1.0) {
            // pow(x, 1) == x exactly (IEEE 754); a sum of integers below 2^24 is exact in f32 in
            // any order, so the reference's sequential sum is the wave's integer sum
            v0 = (float)n0;
            v1 = (float)n1;
            int t = n0 + n1;
#pragma unroll
            for (int o = 32; o; o >>= 1) t += __shfl_xor(t, o);
            sum = (float)t;
        } else {
            if (h0) v0 = (float)pow((double)n0, y);
            if (h1) v1 = (float)pow((double)n1, y);
            for (int i = 0; i < L; ++i) sum += i < 64 ? lane_float(v0, i) : lane_float(v1, i - 64);
        }
        if (sum > 0) {
            v0 = v0 / sum;
            v1 = v1 / sum;
        }
        x0 = (double)v0;
        x1 = (double)v1;
    }
    // The row's entries for the sequential f64 sums below go through this wave's LDS row (entry i at xr[i],
    // read at a uniform address): a load and an add per entry, where the v_readlane pair, the select of the
    // half and the prefix's lane select per entry made the move end VALU-issue bound (round 6; every lane
    // still runs the same additions in the same order)
    __shared__ double s_xrow[kWavesPerBlock][81];
    double *const xr = s_xrow[threadIdx.x >> 6];
    auto stage = [&]() {
        if (h0) xr[lane] = x0;
        if (h1) xr[64 + lane] = x1;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // every lane's stores before any lane's reads
    };
    stage();
    // scores -> float64, renormalised with np.sum (:74-78): np.add.reduce's pairwise block (8
    // accumulators over i = j mod 8, then the remainder), the same additions in every lane
    double tot;
    if (L < 8) {
        tot = 0.0;
        for (int i = 0; i < L; ++i) tot += xr[i];
    } else {
        double r[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = xr[j];
        int i = 8;
        for (; i < L - (L % 8); i += 8)
#pragma unroll
            for (int j = 0; j < 8; ++j) r[j] += xr[i + j];
        tot = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < L; ++i) tot += xr[i];
    }
    x0 = h0 ? ((tot == 0.0) ? 1.0 / (double)L : x0 / tot) : 0.0;
    x1 = h1 ? ((tot == 0.0) ? 1.0 / (double)L : x1 / tot) : 0.0;
    stage();
    // np.random.choice(legal, p=d) (:86): cdf = cumsum; cdf /= cdf[-1]; searchsorted right. The
    // cumsum's prefixes are written over the row in place and land in the lanes of their entries; its last
    // prefix is cdf[-1].
    double acc = 0.0;
    for (int i = 0; i < L; ++i) {
        acc += xr[i];
        xr[i] = acc;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    const double c0 = h0 ? xr[lane] : 0.0, c1 = h1 ? xr[64 + lane] : 0.0;
    const uint64_t b0 = __ballot(h0 && !(c0 / acc <= u)), b1 = __ballot(h1 && !(c1 / acc <= u));
    const int k = b0 ? __builtin_ctzll(b0) : (b1 ? 64 + __builtin_ctzll(b1) : L - 1);  // idx >= L -> L - 1
    // policy target (:81-83): entry i of the row goes to the i-th legal action, the rest are zero
    uint32_t m[3];
    legal_mask(sl.state, m);
    double *const row = sp.ply_policy + ((size_t)s * kMaxPlies + ply) * 81;
    int action = -1;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const int a = lane + 64 * half;
        int rank = 0;
        bool legal = false;
        if (a < 81) {
            const int w = a / 27, b = a % 27;
            legal = (m[w] >> b) & 1u;
            rank = __builtin_popcount(m[w] & ((1u << b) - 1u));
            for (int q = 0; q < w; ++q) rank += __builtin_popcount(m[q]);
        }
        const double e0 = __shfl(x0, rank & 63), e1 = __shfl(x1, rank & 63);
        if (a < 81) row[a] = legal ? (rank < 64 ? e0 : e1) : 0.0;
        const uint64_t hit = __ballot(legal && rank == k);
        if (hit) action = 64 * half + __builtin_ctzll(hit);
    }
    if (lane == 0) {
        sp.mt_pos[s] = pos;
        sp.ply_state[(size_t)s * kMaxPlies + ply] = sl.state;
        sp.ply_action[(size_t)s * kMaxPlies + ply] = (int8_t)action;
        sl.state = next_state(sl.state, action);
        sl.ply = ply + 1;
        if (is_done(sl.state) || sl.ply >= kMaxPlies) {
            sl.finished = 1;
            sl.fin_len = sl.ply;
            sl.fin_game = sl.game;
            sl.fin_value = is_lose(sl.state) ? -1 : 0;  // self_play_cpp.py:95
            sl.live = 0;
        }
        sp.slot[s] = sl;
    }
}

// One block: give finished games arena rows (slot order) and free slots the
// next game ids (slot order) — deterministic for a given slot count.
// host_move (optional, fine-grained pinned): the counters after this move end and the failure word,
// stored at system scope by the kernel itself (the asynchronous move end: no copies on the stream)
__device__ __forceinline__ void store_host_i64(int64_t *p, int64_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
// fail / ctl / err (the asynchronous form): when the search's failure flag is set, the first failed tree
// (lowest slot) and its status go to *err (k_archive skips then) and to host_move[4], and the move is not
// ended (k_move_end changed nothing); the status scan runs only on that rare path (round 6: a k_tree_err
// launch per move scanned every tree's status on the critical path)
__global__ __launch_bounds__(1024) void k_finalize(SelfPlay sp, const int32_t *fail, const TreeCtl *ctl,
                                                   unsigned long long *err, int64_t *host_move) {
    __shared__ unsigned long long wsum[32];
    __shared__ int s_work;  // entries of k_archive's work list
    __shared__ unsigned long long s_first;
    const int tid = threadIdx.x;
    // the counters are read before the scans (only this kernel writes them, after its last barrier): their
    // round trip overlaps the slots' instead of following the scans
    const int64_t arena0 = sp.ctr[2], games0 = sp.ctr[1], next0 = sp.ctr[0];
    const int per = (sp.slots + 1023) / 1024;
    const int b = tid * per, e = min(b + per, sp.slots);
    // the scans need a slot's live / finished / fin_len only: one 16-byte load of Slot bytes 40..55 per slot
    // (up to kFinPer per thread, all in flight together, kept for the second pass), and the second pass
    // reads and rewrites only the slots that change (a game just finished or the slot is free); every other
    // slot was brought up to date by k_move_end. Round 5: the single block read and wrote every 80-byte
    // slot through one CU (31 us per move at 4,096 slots). They go out with the failure word's load (round 6).
    constexpr int kFinPer = 4;
    int4 hot[kFinPer];
#pragma unroll
    for (int j = 0; j < kFinPer; ++j)
        if (b + j < e) hot[j] = *reinterpret_cast<const int4 *>(reinterpret_cast<const char *>(sp.slot + b + j) + 40);
    if (fail && *fail) {
        if (threadIdx.x == 0) s_first = ~0ull;
        __syncthreads();
        for (int t = threadIdx.x; t < sp.slots; t += blockDim.x) {
            const uint32_t st = (uint32_t)ctl[t].status;
            if (st & kErrMask) atomicMin(&s_first, ((unsigned long long)t << 32) | st);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            *err = s_first;
            if (host_move) store_host_i64(host_move + 4, (int64_t)s_first);
        }
        return;
    }
    auto hot_of = [&](int i) -> int4 {
        return i - b < kFinPer ? hot[i - b] : *reinterpret_cast<const int4 *>(reinterpret_cast<const char *>(sp.slot + i) + 40);
    };
    long long fl = 0;
    int fr = 0, fc = 0, first_changed = -1;
    for (int i = b; i < e; ++i) {
        const int4 h = hot_of(i);  // ply, live, finished, fin_len
        if (h.z) {
            fl += h.w;
            ++fc;
        }
        if (!h.y) ++fr;
        if (first_changed < 0 && (h.z || !h.y)) first_changed = i;
    }
    // the thread's first changing slot (usually its only one: ~1 in 40 per move) is loaded whole now, so its
    // round trip runs under the scan instead of after it
    Slot first_slot;
    if (first_changed >= 0) first_slot = sp.slot[first_changed];
    unsigned long long fl_tot, cnt_tot;
    unsigned long long fl_ex = (unsigned long long)fl, cnt_ex = (unsigned long long)fr | ((unsigned long long)fc << 32);
    block_scan2_1024(fl_ex, cnt_ex, &fl_tot, &cnt_tot, wsum);
    long long off = arena0 + (long long)fl_ex;
    int gi = (int)(games0 + (long long)(cnt_ex >> 32));
    int fi = (int)(cnt_ex & 0xFFFFFFFFull);
    const long long fin_total = (long long)fl_tot;
    const int free_total = (int)(cnt_tot & 0xFFFFFFFFull), fin_count = (int)(cnt_tot >> 32);
    if (tid == 0) s_work = 0;
    __syncthreads();
    for (int i = b; i < e; ++i) {
        const int4 h = hot_of(i);
        if (!h.z && h.y) continue;  // playing on: nothing here changes it
        Slot sl = i == first_changed ? first_slot : sp.slot[i];
        if (sl.finished) {
            if (off + sl.fin_len <= sp.arena_cap && gi < sp.games_cap) {
                sl.fin_offset = off;
                GameEntry ge;
                ge.game = sl.fin_game;
                ge.offset = off;
                ge.length = sl.fin_len;
                sp.games[gi] = ge;
            } else {
                sl.fin_offset = -1;  // arena full: host reports UTTT_ERR_CAPACITY
            }
            off += sl.fin_len;
            ++gi;
        }
        if (!sl.live) {
            const int64_t g = next0 + fi;
            ++fi;
            if (g < sp.game_end) {
                sl.state.own[0] = sl.state.own[1] = sl.state.own[2] = 0u;
                sl.state.opp[0] = sl.state.opp[1] = sl.state.opp[2] = 0u;
                sl.state.mains = 0u;
                sl.state.active = -1;
                sl.game = g;
                sl.ply = 0;
                sl.live = 1;
                // the key is seeded by k_archive (one block per slot, so the ~1 in 40 slots refilled per
                // move seed on their own CUs): 624 dependent steps and 624 strided stores per new game
                // on this kernel's single CU were most of its time (round 4)
                sl.seed_pending = 1;
            } else {
                sl.game = -1;
            }
        }
        sp.live[i] = sl.live;
        sp.slot[i] = sl;
        // k_archive's work: a finished game to copy to the arena, or a new game's key to seed (about 1 in
        // 40 slots per move, so k_archive runs a short list instead of a workgroup per slot)
        if ((sl.finished && sl.fin_offset >= 0) || sl.seed_pending) sp.work[1 + atomicAdd(&s_work, 1)] = i;
    }
    __syncthreads();  // every thread read sp.ctr before it is rewritten
    if (tid == 0) {
        sp.work[0] = s_work;
        sp.ctr[2] = arena0 + fin_total;
        sp.ctr[1] = games0 + fin_count;
        const int64_t nxt = next0 + free_total;
        sp.ctr[0] = nxt < sp.game_end ? nxt : sp.game_end;
        // live slots for the next move: those still playing plus the free ones given a game
        sp.ctr[3] = (int64_t)(sp.slots - free_total) + (sp.ctr[0] - next0);
        if (host_move) {
            for (int i = 0; i < 4; ++i) store_host_i64(host_move + i, sp.ctr[i]);
            store_host_i64(host_move + 4, (int64_t)~0ull);
        }
    }
}

// Copy each just-finished game's plies to its arena rows, with values
// (self_play_cpp.py:95-99: ply 0 gets the final value, then alternating), and seed the MT19937
// key of a slot k_finalize gave a new game (numpy's init_genrand(seed_base + game)).
// The seeding wave runs init_genrand's 624-step chain uniformly (every lane the same values, wave-uniform
// operands) and lane i & 63 keeps step i: ten coalesced 64-word stores instead of 624 one-lane stores.
// Round 6: the chain stays in SGPRs (the seed made wave-uniform) and each step's value goes to its lane by one
// v_writelane with an immediate lane index (steps unrolled by template), so a step is five scalar ops and one
// vector op (a compare and a select per step before: 18 us per seed, the move end's longest chain).
template <int J>
__device__ __forceinline__ uint32_t write_lane(uint32_t v, uint32_t x) {
    asm("v_writelane_b32 %0, %1, %2" : "+v"(v) : "s"(x), "i"(J));
    return v;
}
template <int J, int N>
struct SeedSteps {  // init_genrand's steps base + J .. base + N - 1, step base + j into lane j
    static __device__ __forceinline__ void run(uint32_t &x, uint32_t &mine, uint32_t base) {
        x = 1812433253u * (x ^ (x >> 30)) + base + (uint32_t)J;
        mine = write_lane<J>(mine, x);
        SeedSteps<J + 1, N>::run(x, mine, base);
    }
};
template <int N>
struct SeedSteps<N, N> {
    static __device__ __forceinline__ void run(uint32_t &, uint32_t &, uint32_t) {}
};
__device__ __forceinline__ void mt_seed_wave(uint32_t *key, int32_t *pos, uint32_t seed) {
    static_assert(624 == 9 * kWave + 48, "init_genrand's 624 words as 9 full waves and 48");
    const int lane = lane_id();
    uint32_t x = (uint32_t)__builtin_amdgcn_readfirstlane((int)seed);
    uint32_t mine = x;  // key[0] = seed
    SeedSteps<1, kWave>::run(x, mine, 0u);
    key[lane] = mine;
    for (int i0 = kWave; i0 < 9 * kWave; i0 += kWave) {
        SeedSteps<0, kWave>::run(x, mine, (uint32_t)i0);
        key[i0 + lane] = mine;
    }
    SeedSteps<0, 48>::run(x, mine, 9u * kWave);
    if (lane < 48) key[9 * kWave + lane] = mine;
    if (lane == 0) *pos = 624;
}

// Each block: the slots of k_finalize's work list (entry w, w + grid, ...; round 6, in place of a workgroup
// per slot). A finished game's plies are copied with eight independent loads in flight per thread before
// their stores (round 4: one dependent load-store pair per iteration, ~19 memory round trips per game, a
// 39 us launch). seed: the last wave also seeds a refilled slot's key (selfplay_begin and both move ends).
constexpr int kArchiveBlocks = 256;
__global__ __launch_bounds__(256) void k_archive(SelfPlay sp, const unsigned long long *err, int seed) {
    // the failure word, the list's length and this block's first entry are loaded together (the grid is at
    // most the slot count and the list has room for every slot, so entry blockIdx.x is in bounds): one round
    // trip before the first slot load instead of three
    const unsigned long long e0 = err ? *err : ~0ull;
    const int n_work = sp.work[0];
    const int first = sp.work[1 + blockIdx.x];
    if (e0 != ~0ull) return;
    for (int w = blockIdx.x; w < n_work; w += gridDim.x) {
        const int s = w == (int)blockIdx.x ? first : sp.work[1 + w];
        const Slot sl = sp.slot[s];
        const int wave = (int)threadIdx.x >> 6;
        if (seed && sl.seed_pending && wave == 3) {
            mt_seed_wave(sp.mt_key + (size_t)s * 624, sp.mt_pos + s, sp.seed_base + (uint32_t)sl.game);
            if (lane_id() == 0) sp.slot[s].seed_pending = 0;
        }
        if (!sl.finished || sl.fin_offset < 0) continue;
        const size_t src0 = (size_t)s * kMaxPlies, dst0 = (size_t)sl.fin_offset;
        const double *__restrict__ from = sp.ply_policy + src0 * 81;
        double *__restrict__ to = sp.ar_policy + dst0 * 81;
        const int n = sl.fin_len * 81;  // the game's policy rows are contiguous in both places
        constexpr int kU = 8;
        for (int i0 = threadIdx.x; i0 < n; i0 += 256 * kU) {
            double v[kU];
#pragma unroll
            for (int j = 0; j < kU; ++j) v[j] = i0 + 256 * j < n ? from[i0 + 256 * j] : 0.0;
#pragma unroll
            for (int j = 0; j < kU; ++j)
                if (i0 + 256 * j < n) to[i0 + 256 * j] = v[j];
        }
        for (int ply = threadIdx.x; ply < sl.fin_len; ply += 256) {
            sp.ar_state[dst0 + ply] = sp.ply_state[src0 + ply];
            sp.ar_action[dst0 + ply] = sp.ply_action[src0 + ply];
            sp.ar_value[dst0 + ply] = (int8_t)((ply & 1) ? -sl.fin_value : sl.fin_value);
        }
    }
}

static int archive_grid(int slots) { return slots < kArchiveBlocks ? slots : kArchiveBlocks; }

__global__ void k_hwc(const uttt_state_t *st, int64_t n, float *out) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n * 81) return;
    const int64_t row = g / 81;
    const int a = (int)(g % 81);
    const uttt_state_t s = st[row];
    uint32_t m[3];
    legal_mask(s, m);
    float *o = out + row * 243 + image_index(a) * 3;
    o[0] = bit_of(s.own, a) ? 1.0f : 0.0f;
    o[1] = bit_of(s.opp, a) ? 1.0f : 0.0f;
    o[2] = bit_of(m, a) ? 1.0f : 0.0f;
}

}  // namespace uttt

// Root noise (k_root_noise, k_root_priors): the last kernels of the translation unit, behind every kernel of the
// round loop and the move end, whose places in the code object they leave as they were
#include "engine/noise.h"
namespace uttt {
static_assert(offsetof(Slot, ply) == offsetof(Slot, game) + offsetof(NoiseKey, ply) && offsetof(NoiseKey, stream) == 0,
              "k_root_noise reads a slot's game and ply as one NoiseKey");
}  // namespace uttt

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

int uttt_search_begin(uttt_engine_t *e, const uttt_state_t *roots, int32_t n_trees, int32_t sims, int32_t batch) {
    return uttt_search_begin_mode(e, roots, n_trees, sims, batch, UTTT_SEMANTICS_CPP);
}

int uttt_search_begin_mode(uttt_engine_t *e, const uttt_state_t *roots, int32_t n_trees, int32_t sims, int32_t batch,
                           int32_t semantics) {
    if (semantics == UTTT_SEMANTICS_PY)
        if (int rc = refuse_root_noise(e, "uttt_search_begin_mode",
                                       "a py root takes its priors from its first flush: use UTTT_SEMANTICS_CPP"))
            return rc;
    if (int rc = begin_with_semantics(e, "uttt_search_begin_mode", roots, n_trees, sims, batch, semantics)) return rc;
    HIP_TRY(hipMemcpyAsync(e->tr.leaf, roots, sizeof(uttt_state_t) * n_trees, hipMemcpyHostToDevice, e->stream));
    hipLaunchKernelGGL(k_begin, dim3(grid_waves(n_trees)), dim3(kBlock), 0, e->stream, e->pool, e->tr,
                       (const char *)e->tr.leaf, (int)sizeof(uttt_state_t), (const int32_t *)nullptr,
                       (unsigned long long *)nullptr);
    launch_root_noise(e, nullptr, 0);
    return check_launch();
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
    hipLaunchKernelGGL(k_begin, dim3(grid_waves(slots)), dim3(kBlock), 0, e->stream, e->pool, e->tr,
                       (const char *)e->sp.slot, (int)sizeof(Slot), (const int32_t *)e->sp.live, e->d_err.get());
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
