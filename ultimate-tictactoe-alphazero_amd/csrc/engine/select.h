// engine/select.h — the descent: the PUCT scan over a node's child block in groups of 64-child loads, select_wave
// (one wave per tree: descend, back up terminals and evaluation-cache hits in place, queue the first unexpanded
// leaf) and k_select; with them k_select's phase clock, empty in the product build and counting cycles per phase
// under UTTT_DIAG_BUILD.
//
// A part of engine.hip's one translation unit, like its siblings in engine/. The order of the definitions here,
// and of this header among the others, is load-bearing for the code object: engine.hip's include list is the
// order of definition.
#pragma once
#include <cmath>

#include "cache.h"
#include "expand.h"
#include "layout.h"
#include "wave.h"
#include "uttt_bits.h"

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

}  // namespace uttt
