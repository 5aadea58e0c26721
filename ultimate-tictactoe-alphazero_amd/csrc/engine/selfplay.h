// engine/selfplay.h — self-play on the device: Slot, GameEntry and SelfPlay, k_move_end (scores, f64 policy
// target, numpy-legacy MT19937 choice, records), k_finalize (refill + arena offsets), the MT19937 seeding
// templates, k_archive with its grid (archive_grid, a host function), and k_hwc (states -> HWC rows).
//
// A part of engine.hip's one translation unit, like its siblings in engine/. The order of the definitions here,
// and of this header among the others, is load-bearing for the code object: engine.hip's include list is the
// order of definition, which is why k_hwc and archive_grid stay where they stood.
#pragma once
#include <cmath>
#include <cstddef>

#include "evaluators.h"
#include "layout.h"
#include "scan.h"
#include "wave.h"
#include "uttt_bits.h"
#include "uttt_engine.h"

namespace uttt {

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
