// Host sanitizer program for tree reuse: uttt_reroot_host (csrc/rules_api.cpp, csrc/uttt_reroot.h) under
// AddressSanitizer + UBSan. The trees are grown here with the engine's append semantics (a descent by random
// choices to an unexpanded node, k child blocks appended, visits backed up along the path; terminal nodes visited
// in place), so that promoted children with k = 1 and k = 4, unexpanded ones, level-1 duplicates that were never
// expanded and a tree of the largest search (4095 simulations) all occur. Checks what needs no second
// implementation: the output's links stay inside it and ascend (breadth-first order), a node's visits less its k
// are its children's, the root's visits are carried, every visit under the played move is kept, argument errors.
// Buffers are exact-size heap blocks: an out-of-range access is an AddressSanitizer report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "uttt_engine.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {  // xorshift64*
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return (uint32_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 32);
}

static int rec_n(const uint32_t *r) { return (int)(r[2] & 0xFFFFu); }
static int rec_action(const uint32_t *r) { return (int)((r[2] >> 16) & 0x7Fu); }
static int rec_L(const uint32_t *r) { return (int)((r[2] >> 23) & 0x7Fu); }
static int rec_first(const uint32_t *r) { return (int)(r[3] & 0xFFFFFu); }
static int rec_k(const uint32_t *r) { return (int)(r[3] >> 20); }

struct Tree {
    uttt_state_t root;
    std::vector<uint32_t> rec;  // 4 words per node
    int count() const { return (int)(rec.size() / 4); }
};

static void push_block(Tree &t, const uttt_state_t &s) {
    int32_t legal[81];
    const int L = uttt_state_legal_actions(&s, legal);
    const float p = 1.0f / (float)L;
    uint32_t pb;
    std::memcpy(&pb, &p, 4);
    for (int i = 0; i < L; ++i) {
        const uint32_t r[4] = {0u, pb, (uint32_t)legal[i] << 16, 0u};
        t.rec.insert(t.rec.end(), r, r + 4);
    }
}

// sims simulations with flushes of up to `batch` copies from `root`
static Tree grow(const uttt_state_t &root, int sims, int batch) {
    Tree t;
    t.root = root;
    int32_t legal[81];
    const int L0 = uttt_state_legal_actions(&root, legal);
    const uint32_t r0[4] = {0u, 0u, (0x7Fu << 16) | ((uint32_t)L0 << 23), L0 ? (1u | (1u << 20)) : 0u};
    t.rec.assign(r0, r0 + 4);
    if (L0) push_block(t, root);
    for (int done = 0; done < sims && L0;) {
        uttt_state_t s = root;
        std::vector<int> path{0};
        int node = 0;
        for (;;) {
            const uint32_t *r = &t.rec[4 * (size_t)node];
            const int cnt = rec_k(r) * rec_L(r);
            if (!cnt) break;
            // mostly the first copy's moves, as a search's visits concentrate
            const int c = (rnd() % 4) ? (int)(rnd() % (uint32_t)rec_L(r)) : (int)(rnd() % (uint32_t)cnt);
            node = rec_first(r) + c;
            path.push_back(node);
            uttt_state_t nx;
            if (uttt_state_next(&s, rec_action(&t.rec[4 * (size_t)node]), &nx) != UTTT_OK) std::abort();
            s = nx;
        }
        int k = 1;
        if (!uttt_state_is_done(&s)) {
            k = batch < sims - done ? batch : sims - done;
            uint32_t *r = &t.rec[4 * (size_t)node];
            const int L = uttt_state_legal_actions(&s, legal);
            r[2] = (r[2] & ~(0x7Fu << 23)) | ((uint32_t)L << 23);
            r[3] = (uint32_t)t.count() | ((uint32_t)k << 20);
            for (int j = 0; j < k; ++j) push_block(t, s);
        }
        const float v = (float)(rnd() % 5) * 0.25f - 0.5f;
        for (size_t d = 0; d < path.size(); ++d) {
            uint32_t *r = &t.rec[4 * (size_t)path[d]];
            float w;
            std::memcpy(&w, &r[0], 4);
            for (int j = 0; j < k; ++j) w += ((path.size() - 1 - d) & 1) ? -v : v;
            std::memcpy(&r[0], &w, 4);
            r[2] += (uint32_t)k;
        }
        done += k;
    }
    return t;
}

static int failures = 0;
#define CHECK(c)                                              \
    do {                                                      \
        if (!(c)) {                                           \
            ++failures;                                       \
            std::printf("line %d: %s\n", __LINE__, #c);       \
        }                                                     \
    } while (0)

static long long checked = 0, kept_trees = 0, fresh_trees = 0, merged_mixed = 0;

static void reroot_all(const Tree &t, int sims) {
    const uint32_t *root = t.rec.data();
    const int n = t.count(), L0 = rec_L(root);
    for (int i = 0; i < L0; ++i) {
        const uint32_t *c = &t.rec[4 * (size_t)(1 + i)];
        const int a = rec_action(c);
        // exact-size copies of the inputs and an exact-size output
        std::vector<uint32_t> in(t.rec), out((size_t)4 * (size_t)(n > 82 ? n : 82), 0xCDCDCDCDu);
        uttt_state_t st = t.root;
        int32_t m = -1;
        CHECK(uttt_reroot_host(in.data(), n, &st, a, out.data(), &m) == UTTT_OK);
        CHECK(in == t.rec);
        if (m < 1) {
            CHECK(m >= 1);
            continue;
        }
        ++checked;
        const uint32_t *nr = out.data();
        uttt_state_t ns;
        uttt_state_next(&st, a, &ns);
        int32_t legal[81];
        const int Lp = uttt_state_legal_actions(&ns, legal);
        CHECK(rec_L(nr) == Lp && rec_action(nr) == 0x7F && m >= 1 + Lp && m <= (n > 82 ? n : 82));
        const bool keep = rec_k(c) > 0 && rec_L(c) > 0;
        CHECK(rec_n(nr) == (keep ? rec_n(c) - rec_k(c) : 0));
        CHECK(rec_n(nr) <= sims - 1);
        keep ? ++kept_trees : ++fresh_trees;
        if (!keep) CHECK(m == 1 + Lp);
        int sum1 = 0, next_first = 1 + Lp;
        for (int r = 0; r < Lp; ++r) {
            const uint32_t *ch = &out[4 * (size_t)(1 + r)];
            CHECK(rec_action(ch) == legal[r]);
            sum1 += rec_n(ch);
        }
        CHECK(sum1 == rec_n(nr));
        for (int q = 1; q < m; ++q) {  // breadth-first: blocks in the order of their nodes, end to end
            const uint32_t *x = &out[4 * (size_t)q];
            const int cnt = rec_k(x) * rec_L(x);
            if (!cnt) continue;
            CHECK(rec_first(x) == next_first && next_first + cnt <= m);
            if (rec_first(x) != next_first || next_first + cnt > m) break;
            int s = 0;
            for (int j = 0; j < cnt; ++j) s += rec_n(&out[4 * (size_t)(next_first + j)]);
            CHECK(s == rec_n(x) - rec_k(x));
            next_first += cnt;
        }
        CHECK(next_first == m);
        if (keep && rec_k(c) > 1) {  // a move of c with expanded and never expanded duplicates
            const int kc = rec_k(c), fc = rec_first(c);
            for (int r = 0; r < Lp; ++r) {
                int some = 0, all = 1;
                for (int j = 0; j < kc; ++j) {
                    const int kj = rec_k(&t.rec[4 * (size_t)(fc + j * Lp + r)]);
                    some |= kj > 0;
                    all &= kj > 0;
                }
                merged_mixed += some && !all;
            }
        }
    }
    // what is not a move of the root is refused, and nothing is written
    std::vector<uint32_t> out((size_t)4 * (size_t)(n > 82 ? n : 82), 0xCDCDCDCDu);
    int32_t m = -7;
    uttt_state_t st = t.root;
    int32_t legal[81];
    const int L = uttt_state_legal_actions(&st, legal);
    int bad = 0;
    for (int i = 0; i < L && legal[i] == bad; ++i) ++bad;
    const int32_t bads[] = {-1, 81, bad < 81 && L < 81 ? bad : 200};
    for (int32_t a : bads) CHECK(uttt_reroot_host(t.rec.data(), n, &st, a, out.data(), &m) == UTTT_ERR_ARG && m == -7);
    CHECK(uttt_reroot_host(nullptr, n, &st, 0, out.data(), &m) == UTTT_ERR_ARG);
}

int main() {
    uttt_state_t s0;
    uttt_state_initial(&s0);
    // roots: the initial position and positions along random games
    std::vector<uttt_state_t> roots{s0};
    for (int g = 0; g < 6; ++g) {
        uttt_state_t s = s0;
        for (int ply = 0; !uttt_state_is_done(&s); ++ply) {
            int32_t legal[81];
            const int n = uttt_state_legal_actions(&s, legal);
            if (ply % 9 == 4) roots.push_back(s);
            uttt_state_t t;
            if (uttt_state_next(&s, legal[rnd() % (uint32_t)n], &t) != UTTT_OK) return 2;
            s = t;
        }
    }
    const int shapes[][2] = {{16, 1}, {16, 4}, {50, 8}, {33, 5}};
    for (const auto &sh : shapes)
        for (const uttt_state_t &r : roots) reroot_all(grow(r, sh[0], sh[1]), sh[0]);
    // a full-size tree: the largest search an engine runs (its pool holds 82 + 81 * 4095 records)
    {
        const Tree big = grow(s0, UTTT_MAX_SIMS, 8);
        CHECK(big.count() <= 82 + 81 * UTTT_MAX_SIMS && big.count() > 10000);
        reroot_all(big, UTTT_MAX_SIMS);
    }
    CHECK(kept_trees > 100 && fresh_trees > 100 && merged_mixed > 0);
    std::printf("tree reuse host: %lld re-roots (%lld kept a subtree, %lld fresh), %lld mixed duplicate sets, %d failures\n",
                checked, kept_trees, fresh_trees, merged_mixed, failures);
    return failures ? 1 : 0;
}
