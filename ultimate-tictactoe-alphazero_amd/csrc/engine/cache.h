// engine/cache.h — the evaluation cache (EvalCache): an open-addressing table in HBM from a position to the raw
// evaluator output, probed and looked up by k_select, filled by k_apply; the record layout is described below.
#pragma once
#include "layout.h"

namespace uttt {

// ------------------------------------------------------ evaluation cache --
// Open-addressing table in HBM: position (32 B) -> raw evaluator output (81
// priors + value, before legal masking). The evaluator is a pure function of
// the position (the reference feeds it to_input_tensor(), uttt_game.cpp:244),
// so a hit replays exactly what a new evaluation would return. Looked up in
// k_select (a hit is expanded in place: no network round), filled by k_apply.
constexpr int kProbe = 8;
constexpr int kCacheVal = 82;
// One record per slot, three 128-byte lines: the key (32 B), the 82 values (328 B), padding. Written
// and read as 16-byte agent-scope (sc1) accesses, 23 lanes of one wave: one fabric write per 16 B
// instead of one per 4-byte store (MI355X_MICROARCH.md: narrow sc1 stores are one fabric write each).
constexpr int kRecBytes = 384;
constexpr int kRecVal = 32;  // the key is the record's first 32 bytes
constexpr int kRecLanes = 23;  // 16-byte pieces written per record: 2 of key, 21 of values
constexpr int kSc1 = 16;       // buffer-intrinsic cache-policy bit: sc1 (agent scope)
static_assert(kRecVal + 16 * (kRecLanes - 2) >= kRecVal + 4 * kCacheVal && 16 * kRecLanes <= kRecBytes, "record");

struct EvalCache {
    // Per slot one flag word: bits 0-15 a version (0 empty; odd: a writer holds the slot; even >= 2:
    // ready), bits 16-31 the ready entry's tag (16 bits of its position's hash). A writer claims by
    // CAS from the value it saw to that + 1 and publishes the version + 2 with the new tag, so every
    // publish is a new flag value: a reader compares the flag it probed with the flag after its copy
    // (a seqlock without ABA). Probes read only the flags (32 contiguous bytes for 8 slots) and
    // load a record only for a ready slot whose tag matches (round 4: rounds 1-3 read 8 keys per probe).
    uint32_t *flag;
    char *rec;           // [slot][kRecBytes]
    uint32_t mask;       // capacity - 1
    unsigned long long *ctr;  // [0] hits, [1] misses (network leaves), [2] inserts, [3] replacements
};

__device__ __forceinline__ bool flag_ready(uint32_t f) { return (f & 0xFFFFu) != 0u && !(f & 1u); }
__device__ __forceinline__ uint32_t flag_tag(uint32_t f) { return f >> 16; }
// the flag that publishes a slot claimed from flag f (f & 0xFFFF even, or 0 for an empty slot)
__device__ __forceinline__ uint32_t flag_publish(uint32_t f, uint32_t tag) {
    const uint32_t v = (f & 0xFFFFu) + 2u;
    return (tag << 16) | (v > 0xFFFFu ? 2u : v);
}

__device__ __forceinline__ uint64_t state_hash64(const uttt_state_t &s) {
    const uint64_t a = ((uint64_t)s.own[1] << 32) | s.own[0];
    const uint64_t b = ((uint64_t)s.opp[0] << 32) | s.own[2];
    const uint64_t c = ((uint64_t)s.opp[2] << 32) | s.opp[1];
    const uint64_t d = ((uint64_t)(uint32_t)s.active << 32) | s.mains;
    return mix64(mix64(mix64(mix64(kGold ^ a) ^ b) ^ c) ^ d);
}
// a position's tag: the top 16 bits of its hash (its slot: the low 32 bits)
__device__ __forceinline__ uint32_t state_tag(uint64_t h64) { return (uint32_t)(h64 >> 48); }

// 16-byte piece `hi` (0 or 1) of a position's 32-byte key, by selects: indexing the state's words by a
// lane-dependent offset made the state a private array, which the compiler placed in LDS addressed by
// the flat work-item id, i.e. a read of the dispatch packet in host memory at every launch (round 4:
// 2-26 us before k_select's first descent, tools/diag/select_cycles.py)
__device__ __forceinline__ uint4 key_piece(const uttt_state_t &s, bool hi) {
    return make_uint4(hi ? s.opp[1] : s.own[0], hi ? s.opp[2] : s.own[1], hi ? s.mains : s.own[2],
                      hi ? (uint32_t)s.active : s.opp[0]);
}

__device__ __forceinline__ bool same_state(const uttt_state_t &x, const uttt_state_t &y) {
    return x.own[0] == y.own[0] && x.own[1] == y.own[1] && x.own[2] == y.own[2] && x.opp[0] == y.opp[0] &&
           x.opp[1] == y.opp[1] && x.opp[2] == y.opp[2] && x.mains == y.mains && x.active == y.active;
}

// The table may be shared by several engines whose kernels run concurrently on
// other XCDs, whose L2s are not coherent with this one: every access to flag and
// record is agent-scope (sc1: relaxed agent atomics, or buffer accesses with the
// sc1 bit). Entries are exact (the evaluator is a pure function of the position),
// so any ready entry with a matching key is correct; a reader re-checks the flag
// after copying the values, so an entry rewritten meanwhile is never mixed into the copy.
template <typename T>
__device__ __forceinline__ T ld_agent(const T *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <typename T>
__device__ __forceinline__ void st_agent(T *p, T v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

typedef __amdgpu_buffer_rsrc_t rsrc_t;
typedef float floatx4_t __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
// a wave-uniform slot's record as a 384-byte buffer
__device__ __forceinline__ rsrc_t rec_rsrc(const EvalCache &c, uint32_t slot) {
    slot = (uint32_t)__builtin_amdgcn_readfirstlane((int)slot);
    return __builtin_amdgcn_make_buffer_rsrc(c.rec + (size_t)slot * kRecBytes, 0, kRecBytes, 0x00020000);
}

// Wave-uniform lookup: lanes 0..kProbe-1 read the kProbe slots' flags at once; the first ready slot
// whose tag matches (a hit counts only if no empty slot precedes it in probe order) has its whole
// record read in one round trip (lanes 0-1 the key, checked against s; 2-22 the values), then the
// flag is re-checked. On a hit the 82 values are copied to dst (LDS, 16-byte aligned, >= 84 floats)
// and true is returned; a tag that matched another position's entry (a 16-bit collision) is a miss.
// The probe in two halves: the flags' loads are issued first, so work that does not need them (the select's
// leaf checks) runs under their round trip (round 6)
struct CacheProbe {
    uint64_t h64;
    uint32_t f;  // lane l < kProbe: flag of slot h + l
};
__device__ __forceinline__ CacheProbe cache_probe_issue(const EvalCache &c, const uttt_state_t &s) {
    CacheProbe p;
    p.h64 = 0ull;
    p.f = 0u;
    if (!c.flag) return p;
    const int lane = (int)(threadIdx.x & 63);
    p.h64 = state_hash64(s);
    p.f = lane < kProbe ? ld_agent(c.flag + (((uint32_t)p.h64 + (uint32_t)lane) & c.mask)) : 0u;
    return p;
}

__device__ bool cache_lookup_probed(const EvalCache &c, const CacheProbe &pr, const uttt_state_t &s, float *dst) {
    if (!c.flag) return false;
    const int lane = (int)(threadIdx.x & 63);
    const uint64_t h64 = pr.h64;
    const uint32_t h = (uint32_t)h64, tag = state_tag(h64);
    const uint32_t f = pr.f;
    const uint64_t cand = __ballot(lane < kProbe && flag_ready(f) && flag_tag(f) == tag);
    const uint64_t empty = __ballot(lane < kProbe && f == 0u);
    if (!cand) return false;
    const int hl = __builtin_ctzll(cand);
    if (empty && __builtin_ctzll(empty) < hl) return false;
    const uint32_t hs = (h + (uint32_t)hl) & c.mask;
    const uint32_t f1 = (uint32_t)__builtin_amdgcn_readlane((int)f, hl);
    const rsrc_t r = rec_rsrc(c, hs);
    u32x4_t piece = {0u, 0u, 0u, 0u};
    if (lane < kRecLanes) piece = __builtin_amdgcn_raw_buffer_load_b128(r, 16 * lane, 0, kSc1);
    // seqlock read side: the record loads are served before the re-check is issued; any writer
    // that touched the record since the probe bumped the flag first (claim), so the re-check differs
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const uint4 kp = key_piece(s, (lane & 1) != 0);
    const bool key_ok = piece[0] == kp.x && piece[1] == kp.y && piece[2] == kp.z && piece[3] == kp.w;
    if (__ballot(lane < 2 && !key_ok)) return false;
    bool ok = true;
    if (lane == 0) ok = ld_agent(c.flag + hs) == f1;
    if (!__shfl(ok, 0)) return false;
    if (lane >= 2 && lane < kRecLanes) *reinterpret_cast<u32x4_t *>(dst + 4 * (lane - 2)) = piece;
    return true;
}

// Wave-level insert of (s -> 81 priors, value): lane l holds prior l in p0 and prior 64 + l in p1
// (l < 17). Lane 0 claims a slot by CAS (flag -> odd); the record is stored as 23 16-byte sc1
// pieces and drained (s_waitcnt vmcnt(0)) before the new flag is published, so a reader on
// any XCD that sees the flag sees the data. A ready slot with this position's tag counts as this
// position (no insert; a 16-bit collision only costs a missed entry), and a concurrent insert of
// the same key may leave a harmless duplicate. When all kProbe slots hold other positions, one of
// them (chosen by the hash) is replaced. Entries are exact, so the table never needs clearing
// while the evaluator is unchanged: it stays warm across moves. Returns whether a record was written.
// sum >= 0 marks `psum` (the sequential f32 sum of the legal priors, uttt_mcts.cpp:150-153, as
// expand_backup computed it) valid: it is stored beside the values (value 82, with 1.0f at 83), so a
// hit expands without re-adding up to 81 priors one dependent add after another.
constexpr int kRecSum = 82, kRecSumFlag = 83;
// A publish held back by cache_insert (defer): the claimed slot and its flag value, stored by the caller once
// its own later stores are drained anyway (k_round1's end of block), so the record's drain is not a round
// trip of its own on the wave's chain (round 6)
struct CachePublish {
    int32_t slot;  // -1: nothing held
    uint32_t pub;
};
__device__ __forceinline__ void cache_publish(const EvalCache &c, const CachePublish &d) {
    if (d.slot < 0 || (threadIdx.x & 63) != 0) return;
    st_agent(c.flag + d.slot, d.pub);
    atomicAdd(stripe_of(c.ctr + 2 * kRow), 1ull);
}

// pr: the kProbe slots' flags for s, loaded ahead (cache_probe_issue, before the expansion's work)
__device__ bool cache_insert(const EvalCache &c, const CacheProbe &pr, const uttt_state_t &s, float p0, float p1, float v,
                             bool has_sum = false, float psum = 0.0f, CachePublish *defer = nullptr) {
    if (!c.flag) return false;
    const int lane = (int)(threadIdx.x & 63);
    int slot = -1;
    uint32_t pub = 0u;
    // the kProbe slots' flags in one round trip (lanes 0..kProbe-1), then lane 0 acts on the first
    // slot that holds this position's tag or is empty; a lost claim falls back to probing one slot
    // after another from there
    const uint64_t h64 = pr.h64;
    const uint32_t h = (uint32_t)h64, tag = state_tag(h64);
    const uint32_t f = pr.f;
    const uint64_t here = __ballot(lane < kProbe && flag_ready(f) && flag_tag(f) == tag);
    const uint64_t free_ = __ballot(lane < kProbe && f == 0u);
    const uint64_t either = here | free_;
    const int first = either ? __builtin_ctzll(either) : kProbe;
    if (lane == 0) {
        bool present = first < kProbe && ((here >> first) & 1ull);
        int i0 = first;
        if (!present && first < kProbe) {
            const uint32_t sl = (h + (uint32_t)first) & c.mask;
            if (atomicCAS(c.flag + sl, 0u, 1u) == 0u) {
                slot = (int)sl;
                pub = flag_publish(0u, tag);
            } else {
                i0 = first + 1;
            }
        }
        for (int i = i0; slot < 0 && !present && i < kProbe; ++i) {
            const uint32_t sl = (h + (uint32_t)i) & c.mask;
            const uint32_t fi = ld_agent(c.flag + sl);
            if (flag_ready(fi) && flag_tag(fi) == tag) {
                present = true;
                break;
            }
            if (fi == 0u && atomicCAS(c.flag + sl, 0u, 1u) == 0u) {
                slot = (int)sl;
                pub = flag_publish(0u, tag);
                break;
            }
        }
        if (slot < 0 && !present) {  // every probe slot taken: replace one (version v -> v + 1 -> v + 2)
            const uint32_t sl = (h + (h >> 29)) & c.mask;
            const uint32_t fr = ld_agent(c.flag + sl);
            if (flag_ready(fr) && atomicCAS(c.flag + sl, fr, fr + 1u) == fr) {
                slot = (int)sl;
                pub = flag_publish(fr, tag);
                atomicAdd(stripe_of(c.ctr + 3 * kRow), 1ull);
            }
        }
    }
    slot = __shfl(slot, 0);
    if (slot < 0) return false;
    pub = (uint32_t)__builtin_amdgcn_readfirstlane((int)pub);
    // piece j of the record: j < 2 the key's words 4j..4j+3, else values 4(j-2)..4(j-2)+3
    // (value e < 64: lane e's p0; e < 81: lane e-64's p1; e == 81: v)
    floatx4_t piece;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int e = 4 * (lane - 2) + i;
        const float a = __shfl(p0, e & 63);
        const float b = __shfl(p1, (e - 64) & 63);
        piece[i] = e < 64 ? a
                          : (e < 81 ? b
                                    : (e == 81 ? v : (e == kRecSum && has_sum ? psum : (e == kRecSumFlag && has_sum ? 1.0f : 0.0f))));
    }
    if (lane < 2) {
        const uint4 kp = key_piece(s, lane != 0);
        piece = floatx4_t{__uint_as_float(kp.x), __uint_as_float(kp.y), __uint_as_float(kp.z), __uint_as_float(kp.w)};
    }
    const rsrc_t r = rec_rsrc(c, (uint32_t)slot);
    // all 24 pieces (the padding as zeros): the record's three 128-byte lines are written whole, so none is
    // a partial-line write at the memory side (round 6; 23 pieces left the third line 112 of 128 bytes)
    if (lane < kRecBytes / 16)
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, piece), r, 16 * lane, 0, kSc1);
    if (defer) {  // the caller drains and publishes
        defer->slot = slot;
        defer->pub = pub;
        return true;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    cache_publish(c, CachePublish{slot, pub});
    return true;
}

}  // namespace uttt
