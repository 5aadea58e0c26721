// engine/search1.h — a whole one-tree search as one resident wave: Search1Host (the pinned block through which
// the wave and the host meet), kSearch1Timeout and k_search1 (k_begin's, apply_wave's, select_wave's and
// root_scores' bodies in turn).
//
// A part of engine.hip's one translation unit, like its siblings in engine/. The order of the definitions here,
// and of this header among the others, is load-bearing for the code object: engine.hip's include list is the
// order of definition.
#pragma once
#include <cstddef>

#include "apply.h"
#include "cache.h"
#include "evaluators.h"
#include "expand.h"
#include "layout.h"
#include "select.h"
#include "wave.h"
#include "uttt_engine.h"

namespace uttt {

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

}  // namespace uttt
