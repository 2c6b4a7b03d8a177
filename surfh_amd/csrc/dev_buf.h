// Ownership of device memory.  Every device allocation of the library is held by a DevBuf: the buffer is freed when its owner
// goes away (a plan, a table, a call's scope), so no free list is kept by hand and an error return cannot leak.  Rules:
//   owners    DevBuf members and locals.  Move-only: ownership moves by move construction, move assignment or swap.
//   views     raw pointers to memory some DevBuf owns (the tables handed to kernels, aliases of a work vector); each is
//             marked "view" where it is declared and is never freed.
//   lazy sets buffers of a live plan that are allocated on first use go through ensure_set below: all or nothing.
// This header includes no HIP header.  All raw calls go through dev_raw_alloc / dev_raw_free (defined once, in plan.hip; a
// host test supplies its own pair) -- the library calls hipMalloc and hipFree nowhere else, which is what lets
// surfh_debug_alloc_count state "no leak" as an equality.
#pragma once

#include <algorithm>
#include <cstddef>
#include <utility>
#include <vector>

struct ihipStream_t;

namespace surfh_impl __attribute__((visibility("hidden"))) {

int fail(const char *fmt, ...);        // records the message surfh_last_error() returns and returns 1

// 0, or the error recorded through fail() and 1 (*p is then left null)
int dev_raw_alloc(void **p, size_t bytes);
void dev_raw_free(void *p);
// the copies and clears of upload / zeros (plan.hip); null stream + !async: synchronous.  Same contract as dev_raw_alloc.
int dev_raw_upload(void *dst, const void *src, size_t bytes);
int dev_raw_clear(void *p, size_t bytes, ihipStream_t *stream, bool async);

template <typename T>
class DevBuf {
    T *ptr_ = nullptr;

public:
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : ptr_(o.ptr_) { o.ptr_ = nullptr; }
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) {
            reset();
            ptr_ = o.ptr_;
            o.ptr_ = nullptr;
        }
        return *this;
    }
    ~DevBuf() { reset(); }
    void reset() {
        if (ptr_) dev_raw_free(ptr_);
        ptr_ = nullptr;
    }
    void swap(DevBuf &o) noexcept { std::swap(ptr_, o.ptr_); }
    T *get() const { return ptr_; }
    operator T *() const { return ptr_; }      // call sites read an owner like the pointer it holds; truth tests included

    // n elements (at least one, so that an empty table still has an address); a buffer that holds something is never re-allocated
    int alloc(size_t n) {
        if (ptr_) return fail("internal: allocation into a device buffer that is already allocated");
        return dev_raw_alloc((void **)&ptr_, std::max<size_t>(n, 1) * sizeof(T));
    }
    int upload(const std::vector<T> &h) {
        if (alloc(h.size())) return 1;
        return h.empty() ? 0 : dev_raw_upload(ptr_, h.data(), h.size() * sizeof(T));
    }
    int zeros(size_t n) { return alloc(n) || dev_raw_clear(ptr_, n * sizeof(T), nullptr, false); }
    int zeros(size_t n, ihipStream_t *stream) { return alloc(n) || dev_raw_clear(ptr_, n * sizeof(T), stream, true); }
};

// ---- lazy sets ----------------------------------------------------------------------------------------------------------------
// One member of a set: the plan's buffer and its size, or the host vector it is uploaded from.
template <typename T>
struct SetMember {
    DevBuf<T> *dst;
    size_t n;
    const std::vector<T> *src;
    DevBuf<T> tmp;
    int build() { return src ? tmp.upload(*src) : tmp.alloc(n); }
};
template <typename T>
SetMember<T> member(DevBuf<T> &d, size_t n) { return {&d, n, nullptr, {}}; }
template <typename T>
SetMember<T> member(DevBuf<T> &d, const std::vector<T> &h) { return {&d, 0, &h, {}}; }

// Allocates the set unless every member is there already.  The buffers are built in locals, in the order given; `setup` (the
// launch that fills one, a clear) then gets their pointers in that order and returns 0 or an error.  Only after all of that are
// they moved into the plan: on failure the locals free themselves and the plan is exactly as before the call.
template <typename Setup, typename... Ts>
int ensure_set_with(Setup &&setup, SetMember<Ts>... m) {
    if ((... && (m.dst->get() != nullptr))) return 0;
    if ((... || m.build())) return 1;
    if (setup(m.tmp.get()...)) return 1;
    (..., m.dst->swap(m.tmp));
    return 0;
}
template <typename... Ts>
int ensure_set(SetMember<Ts>... m) {
    return ensure_set_with([](Ts *...) { return 0; }, std::move(m)...);
}

}  // namespace surfh_impl
