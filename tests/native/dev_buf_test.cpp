// Stand-alone host test of surfh_amd/csrc/dev_buf.h: the owner type and the lazy-set helper, on an allocator built on malloc that
// counts what is live and can refuse its k-th call.  tests/test_dev_buf_host.py compiles and runs it (no GPU, no HIP).
#include "../../surfh_amd/csrc/dev_buf.h"

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>

using namespace surfh_impl;

namespace {
std::set<void *> g_live;      // a free of something not in here is a double free or a stray pointer
long g_total = 0, g_fail_at = 0, g_fails = 0, g_checks = 0;
char g_msg[256];
}  // namespace

namespace surfh_impl {
int fail(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_msg, sizeof g_msg, fmt, ap);
    va_end(ap);
    ++g_fails;
    return 1;
}
int dev_raw_alloc(void **p, size_t bytes) {
    *p = nullptr;
    if (++g_total == g_fail_at) {
        g_fail_at = 0;
        return fail("out of memory (injected)");
    }
    if (bytes == 0) return fail("zero-byte allocation");
    *p = malloc(bytes);
    g_live.insert(*p);
    return 0;
}
void dev_raw_free(void *p) {
    if (!p) return;
    if (!g_live.erase(p)) {
        fprintf(stderr, "FAILED: free of a pointer that is not live\n");
        exit(1);
    }
    free(p);
}
// the copies and clears behind upload() and zeros(): host memory here
int dev_raw_upload(void *dst, const void *src, size_t bytes) {
    memcpy(dst, src, bytes);
    return 0;
}
int dev_raw_clear(void *p, size_t bytes, ihipStream_t *, bool) {
    memset(p, 0, bytes);
    return 0;
}
}  // namespace surfh_impl

#define CHECK(c)                                                          \
    do {                                                                  \
        ++g_checks;                                                       \
        if (!(c)) {                                                       \
            fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            exit(1);                                                      \
        }                                                                 \
    } while (0)

static void arm(long k) { g_fail_at = k ? g_total + k : 0; }
static size_t live() { return g_live.size(); }

static void test_owner() {
    const size_t base = live();
    {
        DevBuf<float> a;
        CHECK(!a && a.get() == nullptr);
        CHECK(a.alloc(7) == 0 && a && live() == base + 1);
        float *raw = a;                        // reads like the pointer it holds
        CHECK(raw == a.get());
        raw[6] = 1.f;                          // 7 elements are there (the sanitizer watches)
        a.reset();
        CHECK(!a && live() == base);
        a.reset();                             // a second reset frees nothing
        CHECK(live() == base);
        CHECK(a.alloc(3) == 0 && live() == base + 1);
    }                                          // the destructor frees, once
    CHECK(live() == base);
    {   // moves and swap
        DevBuf<int> a, c;
        CHECK(a.alloc(4) == 0);
        int *raw = a;
        DevBuf<int> b(std::move(a));
        CHECK(!a && b.get() == raw && live() == base + 1);
        CHECK(c.alloc(2) == 0 && live() == base + 2);
        int *rc = c;
        c = std::move(b);                      // what c held is freed, b is empty
        CHECK(!b && c.get() == raw && live() == base + 1 && !g_live.count(rc));
        c.swap(a);
        CHECK(!c && a.get() == raw && live() == base + 1);
    }
    CHECK(live() == base);
    {   // alloc on a full buffer is refused and leaks nothing
        DevBuf<double> a;
        CHECK(a.alloc(5) == 0);
        double *raw = a;
        const long fails = g_fails, total = g_total;
        CHECK(a.alloc(5) == 1 && g_fails == fails + 1 && g_total == total);
        CHECK(a.get() == raw && live() == base + 1);
    }
    CHECK(live() == base);
    {   // alloc(0) still allocates one element
        DevBuf<double> a;
        CHECK(a.alloc(0) == 0 && a);
        a[0] = 2.0;
        CHECK(live() == base + 1);
    }
    CHECK(live() == base);
    {   // a refused allocation leaves the buffer empty
        DevBuf<float> a;
        arm(1);
        CHECK(a.alloc(9) == 1 && !a && live() == base);
        CHECK(a.alloc(9) == 0 && a);
    }
    CHECK(live() == base);
    {   // upload and zeros allocate, then fill; an empty vector still gets its one element
        const std::vector<int> h = {3, 1, 4, 1, 5}, none;
        DevBuf<int> a, b, z;
        CHECK(a.upload(h) == 0 && a[0] == 3 && a[4] == 5);
        CHECK(b.upload(none) == 0 && b);
        CHECK(z.zeros(6) == 0 && z[0] == 0 && z[5] == 0);
        CHECK(live() == base + 3);
        CHECK(a.upload(h) == 1 && z.zeros(6) == 1 && live() == base + 3);      // full buffers: refused
    }
    CHECK(live() == base);
}

// a plan's lazy set: five buffers and one set-up step, through the helper the library uses
namespace {
struct Plan {
    DevBuf<float> x, r, d;
    DevBuf<double> sc;
    DevBuf<int> idx;
    bool any() const { return x || r || d || sc || idx; }
    bool all() const { return x && r && d && sc && idx; }
};
}  // namespace
static int g_setup_calls = 0;
static int build_set(Plan &p, bool setup_fails) {
    return ensure_set_with(
        [&](float *x, float *r, float *d, double *sc, int *idx) {
            ++g_setup_calls;
            if (!(x && r && d && sc && idx)) return fail("set-up step saw a missing buffer");
            if (setup_fails) return fail("set-up step failed (injected)");
            x[9] = r[9] = d[9] = 0.f;
            sc[2] = 0.0;
            idx[0] = 1;
            return 0;
        },
        member(p.x, 10), member(p.r, 10), member(p.d, 10), member(p.sc, 3), member(p.idx, 0));
}

static void test_lazy_set() {
    const size_t base = live();
    for (int k = 1; k <= 6; ++k) {             // k = 1..5: the k-th allocation is refused; 6: the set-up step fails
        Plan p;
        const int setups = g_setup_calls;
        if (k <= 5) arm(k);
        CHECK(build_set(p, k == 6) == 1);
        CHECK(!p.any() && live() == base);     // nothing published, nothing leaked
        CHECK(g_setup_calls == setups + (k == 6 ? 1 : 0));
        arm(0);
        CHECK(build_set(p, false) == 0);       // a second, unarmed attempt: a complete set
        CHECK(p.all() && live() == base + 5);
        const long total = g_total;
        const float *x = p.x;
        CHECK(build_set(p, false) == 0);       // present: allocates nothing, runs no set-up, moves nothing
        CHECK(g_total == total && p.x.get() == x && live() == base + 5 && g_setup_calls == setups + (k == 6 ? 2 : 1));
    }
    CHECK(live() == base);
    {   // the plain form, and a set of one
        Plan p;
        arm(2);
        CHECK(ensure_set(member(p.x, 4), member(p.sc, 4)) == 1 && !p.any() && live() == base);
        CHECK(ensure_set(member(p.x, 4), member(p.sc, 4)) == 0 && p.x && p.sc && live() == base + 2);
        CHECK(ensure_set(member(p.idx, 1)) == 0 && p.idx && live() == base + 3);
    }
    CHECK(live() == base);
    {   // members uploaded from host vectors
        const std::vector<int> h = {7, 8, 9};
        Plan p;
        arm(2);
        CHECK(ensure_set(member(p.idx, h), member(p.x, 4)) == 1 && !p.any() && live() == base);
        CHECK(ensure_set(member(p.idx, h), member(p.x, 4)) == 0 && p.idx[2] == 9 && p.x && live() == base + 2);
    }
    CHECK(live() == base);
}

int main() {
    test_owner();
    test_lazy_set();
    if (!g_live.empty()) {
        fprintf(stderr, "FAILED: %zu allocations still live at exit\n", g_live.size());
        return 1;
    }
    printf("dev_buf_test: %ld checks passed, %ld allocations, none live\n", g_checks, g_total);
    return 0;
}
