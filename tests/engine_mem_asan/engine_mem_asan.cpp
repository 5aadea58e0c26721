// Host sanitizer program for the engine's owning buffer type (csrc/engine_mem.h) under AddressSanitizer (with
// leak detection) + UBSan. The allocate / free policy is malloc / free with a count of live blocks, and can be
// told to fail the N-th allocation from now: a block freed twice, used after a failed growth or never freed
// is a sanitizer report, and the count must be back at zero after every case.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "engine_mem.h"

static int g_errors_set = 0;
namespace uttt {
void set_error(const char *, ...) { ++g_errors_set; }
}  // namespace uttt

struct CountedMem {
    static int live, fail_in;  // fail_in: 1 fails the next allocation, 2 the one after it, 0 none
    static void *alloc(size_t bytes) {
        if (fail_in > 0 && --fail_in == 0) {
            uttt::set_error("allocation of %zu bytes failed (as asked)", bytes);
            return nullptr;
        }
        ++live;
        return std::malloc(bytes ? bytes : 1);  // exact size: a store past n elements is a report
    }
    static void free(void *p) {
        --live;
        std::free(p);
    }
};
int CountedMem::live = 0;
int CountedMem::fail_in = 0;

template <typename T>
using TestBuf = uttt::Buf<T, CountedMem>;

static int failures = 0;
#define CHECK(c)                                                     \
    do {                                                             \
        if (!(c)) {                                                  \
            ++failures;                                              \
            std::printf("engine_mem_asan: line %d: %s\n", __LINE__, #c); \
        }                                                            \
    } while (0)

template <typename T>
static void fill(TestBuf<T> &b) {  // every element written and read back
    for (int64_t i = 0; i < b.cap(); ++i) b[i] = (T)i;
    for (int64_t i = 0; i < b.cap(); ++i) CHECK(b.get()[i] == (T)i);
}

int main() {
    {  // grow, regrow (larger, smaller), destroy
        TestBuf<int32_t> b;
        CHECK(b.get() == nullptr && b.cap() == 0);
        CHECK(b.grow(100) == UTTT_OK && b.cap() == 100 && CountedMem::live == 1);
        fill(b);
        CHECK(b.grow(1000) == UTTT_OK && b.cap() == 1000 && CountedMem::live == 1);
        fill(b);
        CHECK(b.grow(7) == UTTT_OK && b.cap() == 7 && CountedMem::live == 1);
        fill(b);
    }
    CHECK(CountedMem::live == 0);
    {  // reset, twice, then the destructor: one free
        TestBuf<double> b;
        CHECK(b.grow(81) == UTTT_OK);
        b.reset();
        b.reset();
        CHECK(b.get() == nullptr && b.cap() == 0 && CountedMem::live == 0);
    }
    CHECK(CountedMem::live == 0);
    {  // a failing grow leaves the buffer empty (the old block freed once); the next grow and the destructor are clean
        TestBuf<int64_t> b;
        CHECK(b.grow(64) == UTTT_OK);
        const int errs = g_errors_set;
        CountedMem::fail_in = 1;
        CHECK(b.grow(128) == UTTT_ERR_HIP);
        CHECK(b.get() == nullptr && b.cap() == 0 && CountedMem::live == 0 && g_errors_set == errs + 1);
        CHECK(b.grow(128) == UTTT_OK && b.cap() == 128 && CountedMem::live == 1);
        fill(b);
        CountedMem::fail_in = 1;
        CHECK(b.grow(256) == UTTT_ERR_HIP && b.get() == nullptr && b.cap() == 0);
    }  // destroyed empty
    CHECK(CountedMem::live == 0);
    {  // a group of three: grown, regrown, then the second allocation of a regrowth fails
        TestBuf<float> pol, val;
        TestBuf<int32_t> base;
        int64_t rows = 0;
        CHECK(uttt::grow_group(rows, 1024, pol, 1024 * 81, val, 1024, base, 1024) == UTTT_OK);
        CHECK(rows == 1024 && pol.cap() == 1024 * 81 && val.cap() == 1024 && base.cap() == 1024 && CountedMem::live == 3);
        fill(pol);
        fill(val);
        fill(base);
        CHECK(uttt::grow_group(rows, 2048, pol, 2048 * 81, val, 2048, base, 4096) == UTTT_OK);
        CHECK(rows == 2048 && base.cap() == 4096 && CountedMem::live == 3);
        fill(base);
        CountedMem::fail_in = 2;
        CHECK(uttt::grow_group(rows, 4096, pol, 4096 * 81, val, 4096, base, 4096) == UTTT_ERR_HIP);
        CHECK(rows == 0 && CountedMem::live == 0);
        CHECK(pol.get() == nullptr && pol.cap() == 0 && val.get() == nullptr && val.cap() == 0);
        CHECK(base.get() == nullptr && base.cap() == 0);  // (it still held its old block when the second failed)
        for (int at = 1; at <= 3; ++at) {  // each position of the failure, from an empty and from a full group
            CountedMem::fail_in = at;
            CHECK(uttt::grow_group(rows, 16, pol, 16 * 81, val, 16, base, 16) == UTTT_ERR_HIP);
            CHECK(rows == 0 && CountedMem::live == 0 && !pol && !val && !base);
            CHECK(uttt::grow_group(rows, 16, pol, 16 * 81, val, 16, base, 16) == UTTT_OK && rows == 16);
            CHECK(CountedMem::live == 3);
            fill(pol);
        }
        CountedMem::fail_in = 2;
        CHECK(uttt::grow_group(rows, 32, pol, 32 * 81, val, 32, base, 32) == UTTT_ERR_HIP && rows == 0);
    }  // destroyed after the failure: nothing is freed twice
    CHECK(CountedMem::live == 0 && CountedMem::fail_in == 0);
    std::printf("engine_mem_asan: %d live blocks, %d errors reported, %d failures\n", CountedMem::live, g_errors_set,
                failures);
    return failures ? 1 : 0;
}
