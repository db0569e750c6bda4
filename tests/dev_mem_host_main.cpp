// Host test of csrc/dev_mem.h (tests/test_dev_mem_cpu.py builds and runs it).  The five HIP calls the header makes are
// defined here over malloc and a table of live pointers, each tagged device / pinned; the n-th allocation can be made to
// fail.  Exit status 0 and "ok", or the first failed check on stderr and status 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

#include "../mvsmplfitting_amd/csrc/dev_mem.h"

using namespace mvfit;

namespace {
enum Kind { DEVICE, PINNED };
struct Block { Kind kind; size_t bytes; };
const size_t GUARD = 16;                 // bytes behind every block, filled like the block with 0xAB
std::map<void*, Block> g_live;
std::vector<size_t> g_live_at_alloc;     // live blocks at every allocation call
int g_allocs = 0, g_fail_at = -1;        // allocation calls so far; the call (counted from 0) that fails
int g_misuse = 0;                        // frees of unknown pointers or through the wrong call, memsets out of a block

hipError_t stub_alloc(void** out, size_t bytes, Kind kind) {
    g_live_at_alloc.push_back(g_live.size());
    if (g_allocs++ == g_fail_at) return hipErrorOutOfMemory;      // (*out is left as it was, like the runtime)
    unsigned char* p = static_cast<unsigned char*>(malloc(bytes + GUARD));
    memset(p, 0xAB, bytes + GUARD);
    g_live[p] = Block{kind, bytes};
    *out = p;
    return hipSuccess;
}
hipError_t stub_free(void* p, Kind kind) {
    auto it = g_live.find(p);
    if (it == g_live.end() || it->second.kind != kind) { ++g_misuse; return hipErrorInvalidValue; }
    g_live.erase(it);
    free(p);
    return hipSuccess;
}
void start(int fail_at = -1) { g_allocs = 0; g_fail_at = fail_at; g_live_at_alloc.clear(); }

#define CHECK(cond)                                                             \
    do {                                                                        \
        if (!(cond)) {                                                          \
            fprintf(stderr, "dev_mem: line %d: %s\n", __LINE__, #cond);         \
            exit(1);                                                            \
        }                                                                       \
    } while (0)
#define CLEAN() CHECK(g_live.empty() && g_misuse == 0)

bool all_bytes(const void* p, size_t n, unsigned char v) {
    for (size_t i = 0; i < n; ++i) if (static_cast<const unsigned char*>(p)[i] != v) return false;
    return true;
}
}  // namespace

extern "C" {
hipError_t hipMalloc(void** p, size_t bytes) { return stub_alloc(p, bytes, DEVICE); }
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned int) { return stub_alloc(p, bytes, PINNED); }
hipError_t hipFree(void* p) { return stub_free(p, DEVICE); }
hipError_t hipHostFree(void* p) { return stub_free(p, PINNED); }
hipError_t hipMemset(void* p, int v, size_t bytes) {
    auto it = g_live.find(p);
    if (it == g_live.end() || it->second.kind != DEVICE || bytes > it->second.bytes) { ++g_misuse; return hipErrorInvalidValue; }
    memset(p, v, bytes);
    return hipSuccess;
}
}

static void test_pool() {
    {   // scope end frees everything
        start();
        DevPool pool;
        float* a = nullptr; int* b = nullptr;
        CHECK(pool.alloc(&a, 40) == hipSuccess && pool.alloc(&b, 12) == hipSuccess && a && b);
        CHECK(g_live.size() == 2);
    }
    CLEAN();
    {   // release() frees everything, twice is harmless, the pool is usable afterwards
        start();
        DevPool pool;
        char *a = nullptr, *b = nullptr, *c = nullptr;
        CHECK(pool.alloc(&a, 1) == hipSuccess && pool.alloc(&b, 2) == hipSuccess);
        pool.release();
        CLEAN();
        pool.release();
        CLEAN();
        CHECK(pool.alloc(&c, 3) == hipSuccess && g_live.size() == 1);
    }
    CLEAN();
    const int n = 4;
    for (int k : {0, 1, n - 1}) {       // the k-th alloc fails: error returned, out-pointer null, the earlier ones still freed
        start(k);
        {
            DevPool pool;
            char* p[n];
            for (int i = 0; i < n; ++i) {
                p[i] = reinterpret_cast<char*>(0x1);
                const hipError_t e = pool.alloc(&p[i], 8 + i, true);
                CHECK((e != hipSuccess) == (i == k));
                CHECK((p[i] == nullptr) == (i == k));
            }
            CHECK(g_live.size() == (size_t)n - 1);
        }
        CLEAN();
    }
    {   // zero fills exactly the requested bytes; without it the block is left as allocated
        start();
        DevPool pool;
        unsigned char *z = nullptr, *u = nullptr;
        CHECK(pool.alloc(&z, 37, true) == hipSuccess && pool.alloc(&u, 37) == hipSuccess);
        CHECK(all_bytes(z, 37, 0) && all_bytes(z + 37, GUARD, 0xAB));
        CHECK(all_bytes(u, 37 + GUARD, 0xAB));
    }
    CLEAN();
    {   // moves: ownership goes over, the target's old contents are freed, nothing twice
        start();
        DevPool a;
        char *p = nullptr, *q = nullptr;
        CHECK(a.alloc(&p, 5) == hipSuccess);
        DevPool b(std::move(a));
        a.release();
        CHECK(g_live.count(p) == 1);
        DevPool c;
        CHECK(c.alloc(&q, 6) == hipSuccess);
        c = std::move(b);
        CHECK(g_live.count(q) == 0 && g_live.count(p) == 1 && g_misuse == 0);
        b.release();
        CHECK(g_live.count(p) == 1);
    }
    CLEAN();
}

template <bool Pinned>
static void test_buf() {
    const Kind kind = Pinned ? PINNED : DEVICE;
    {
        start();
        GrowBuf<Pinned> buf;
        CHECK(buf.get() == nullptr && buf.size() == 0);
        CHECK(buf.reserve(0) == hipSuccess && buf.get() == nullptr && g_allocs == 0);
        CHECK(buf.reserve(100) == hipSuccess && buf.size() == 100 && g_live.size() == 1);
        void* p = buf.get();
        CHECK(p && buf.template as<int>() == static_cast<int*>(p) && g_live[p].kind == kind && g_live[p].bytes == 100);
        // smaller or equal: the address stays, nothing is allocated
        CHECK(buf.reserve(100) == hipSuccess && buf.reserve(7) == hipSuccess && buf.get() == p && buf.size() == 100 && g_allocs == 1);
        // larger: freed BEFORE the new allocation (nothing live at that call)
        CHECK(buf.reserve(101) == hipSuccess && buf.size() == 101 && g_live.size() == 1 && g_live.count(buf.get()) == 1);
        CHECK(g_live_at_alloc.size() == 2 && g_live_at_alloc[0] == 0 && g_live_at_alloc[1] == 0);
        // a failed growth leaves it empty; a later reserve works
        g_fail_at = g_allocs;
        CHECK(buf.reserve(500) != hipSuccess && buf.get() == nullptr && buf.size() == 0 && g_live.empty());
        CHECK(buf.reserve(50) == hipSuccess && buf.size() == 50 && g_live.size() == 1);
        buf.reset();
        CHECK(buf.get() == nullptr && buf.size() == 0);
        CLEAN();
        buf.reset();
        CLEAN();
        CHECK(buf.reserve(9) == hipSuccess);
    }
    CLEAN();                                // (freed at scope end, and only through its own kind's call: g_misuse)
    {   // moves
        start();
        GrowBuf<Pinned> a;
        CHECK(a.reserve(10) == hipSuccess);
        void* p = a.get();
        GrowBuf<Pinned> b(std::move(a));
        CHECK(a.get() == nullptr && a.size() == 0 && b.get() == p && b.size() == 10);
        GrowBuf<Pinned> c;
        CHECK(c.reserve(20) == hipSuccess);
        void* q = c.get();
        c = std::move(b);
        CHECK(g_live.count(q) == 0 && g_live.count(p) == 1 && c.get() == p && c.size() == 10 && b.get() == nullptr);
        CHECK(g_misuse == 0);
    }
    CLEAN();
}

int main() {
    test_pool();
    test_buf<false>();
    test_buf<true>();
    printf("ok\n");
    return 0;
}
