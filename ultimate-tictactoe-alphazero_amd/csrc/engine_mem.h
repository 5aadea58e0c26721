// engine_mem.h — the one owner type for the engine's device and pinned host memory.
//
// Buf<T, Mem> holds a typed pointer and an element capacity, frees in its destructor and cannot be copied, so
// a block has exactly one owner and uttt_engine_destroy needs no list of what to free. Mem is the allocate /
// free pair (engine.hip: hipMalloc / hipFree, hipHostMalloc / hipHostFree; the sanitizer test: counted malloc):
//   static void *alloc(size_t bytes);  nullptr on failure, after reporting it through set_error
//   static void free(void *p);
// No HIP header is needed here: the host sanitizer program (tests/engine_mem_asan) compiles this file alone.
#pragma once
#include <cstddef>
#include <cstdint>

#include "uttt_engine.h"

namespace uttt {

template <typename T, typename Mem>
class Buf {
  public:
    Buf() = default;
    Buf(const Buf &) = delete;
    Buf &operator=(const Buf &) = delete;
    ~Buf() { reset(); }

    T *get() const { return p_; }
    operator T *() const { return p_; }
    T *operator->() const { return p_; }
    int64_t cap() const { return cap_; }  // elements

    void reset() {
        if (p_) Mem::free(p_);
        p_ = nullptr;
        cap_ = 0;
    }
    // Frees the old block, then allocates n elements (contents are not kept). A failure leaves the buffer
    // empty (null, capacity 0), never a freed pointer: the next grow, and the destructor, start clean.
    int grow(int64_t n) {
        reset();
        p_ = static_cast<T *>(Mem::alloc((size_t)n * sizeof(T)));
        if (!p_) return UTTT_ERR_HIP;
        cap_ = n;
        return UTTT_OK;
    }

  private:
    T *p_ = nullptr;
    int64_t cap_ = 0;
};

// Buffers that are sized together grow together: grow_group(cap, n, a, na, b, nb, ...) grows a to na elements,
// b to nb, ..., then sets the group's capacity field to n. On any failure every buffer of the group is reset
// (those before the failed one, and those after it, which still held their old blocks) and cap is 0, so no
// caller ever sees a capacity that some buffer of the group does not have.
inline int grow_each(int rc) { return rc; }
template <typename B, typename... Rest>
int grow_each(int rc, B &b, int64_t n, Rest &&...rest) {
    if (!rc) rc = b.grow(n);
    rc = grow_each(rc, rest...);
    if (rc) b.reset();
    return rc;
}
template <typename... Pairs>
int grow_group(int64_t &cap, int64_t n, Pairs &&...pairs) {
    cap = 0;
    const int rc = grow_each(UTTT_OK, pairs...);
    if (!rc) cap = n;
    return rc;
}

}  // namespace uttt
