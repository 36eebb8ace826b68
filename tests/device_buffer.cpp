// device_buffer.cpp — DeviceBuffer (csrc/device_memory.hpp) against a counting
// host allocator: built by tests/test_device_buffer.py with g++ and
// -fsanitize=address,undefined, run as a child; prints "ok" when every check
// holds.  RTC_DEVICE_MEMORY_NO_HIP leaves the HIP policies, Event and Stream
// out, so no HIP header is needed.
#define RTC_DEVICE_MEMORY_NO_HIP
#include "../ray-tracer-challenge-rs_amd/csrc/device_memory.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <type_traits>

namespace {

constexpr int kErrAlloc = 7;  // what the allocator returns when told to fail

struct Counting {
    static inline int allocs = 0, frees = 0, fail_next = 0;
    static inline size_t last_bytes = 0;
    static inline std::set<void*> live;
    static inline int peak_live = 0;
    static int allocate(void** p, size_t bytes) {
        if (fail_next > 0) {
            --fail_next;
            return kErrAlloc;
        }
        *p = std::malloc(bytes ? bytes : 1);
        if (!*p) return kErrAlloc;
        std::memset(*p, 0xA5, bytes);
        ++allocs;
        last_bytes = bytes;
        live.insert(*p);
        if ((int)live.size() > peak_live) peak_live = (int)live.size();
        return 0;
    }
    static void free(void* p) {
        if (!live.erase(p)) {
            std::printf("FAIL free of a block that is not live\n");
            std::exit(1);
        }
        ++frees;
        std::free(p);
    }
};

using Buf = rtc::DeviceBuffer<unsigned int, Counting>;

int g_checks = 0;
#define CHECK(cond)                                                  \
    do {                                                             \
        ++g_checks;                                                  \
        if (!(cond)) {                                               \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                            \
        }                                                            \
    } while (0)

void reserve_rules() {
    Buf b;
    CHECK(b.get() == nullptr && b.capacity() == 0);
    bool grew = true;
    CHECK(b.reserve(0, &grew) == 0 && !grew && Counting::allocs == 0);  // nothing asked, nothing done
    CHECK(b.reserve(10, &grew) == 0 && grew);
    CHECK(b.get() != nullptr && b.capacity() == 10 && Counting::last_bytes == 10 * sizeof(unsigned int));
    b.get()[9] = 1u;  // (the sanitizer checks the block is as large as it says)
    // within capacity: no allocation, no free, grew == false, the same block
    unsigned int* p = b.get();
    const int a0 = Counting::allocs, f0 = Counting::frees;
    for (size_t n : {(size_t)10, (size_t)3, (size_t)0}) {
        grew = true;
        CHECK(b.reserve(n, &grew) == 0 && !grew);
        CHECK(b.get() == p && b.capacity() == 10 && Counting::allocs == a0 && Counting::frees == f0);
    }
    CHECK(b.reserve(5) == 0 && b.get() == p);  // (grew is optional)
    // growing: the old block is freed before the new one is allocated
    Counting::peak_live = (int)Counting::live.size();
    CHECK(Counting::peak_live == 1);
    CHECK(b.reserve(1000, &grew) == 0 && grew);
    CHECK(b.capacity() == 1000 && Counting::allocs == a0 + 1 && Counting::frees == f0 + 1);
    CHECK(Counting::peak_live == 1 && Counting::live.size() == 1);
    b.get()[999] = 2u;
    // a failed allocation: empty, the error returned, and the next reserve works
    Counting::fail_next = 1;
    grew = false;
    CHECK(b.reserve(2000, &grew) == kErrAlloc && grew);  // (the old contents are gone: the caller must know)
    CHECK(b.get() == nullptr && b.capacity() == 0 && Counting::live.empty());
    CHECK(Counting::frees == f0 + 2 && Counting::allocs == a0 + 1);
    CHECK(b.reserve(4, &grew) == 0 && grew && b.capacity() == 4 && b.get() != nullptr);
    Counting::fail_next = 1;  // a failure on an empty buffer frees nothing
    Buf e;
    const int f1 = Counting::frees;
    CHECK(e.reserve(1) == kErrAlloc && e.get() == nullptr && e.capacity() == 0 && Counting::frees == f1);
}

void moves() {
    const int a0 = Counting::allocs, f0 = Counting::frees;
    {
        Buf a;
        CHECK(a.reserve(8) == 0);
        unsigned int* pa = a.get();
        Buf b(std::move(a));  // construction: the block moves, nothing is freed
        CHECK(b.get() == pa && b.capacity() == 8 && a.get() == nullptr && a.capacity() == 0);
        CHECK(Counting::frees == f0);
        Buf c;
        CHECK(c.reserve(16) == 0);
        unsigned int* pc = c.get();
        b = std::move(c);  // assignment: the target's old block is freed exactly once
        CHECK(b.get() == pc && b.capacity() == 16 && c.get() == nullptr && c.capacity() == 0);
        CHECK(Counting::frees == f0 + 1 && !Counting::live.count(pa) && Counting::live.count(pc));
        Buf& self = b;
        b = std::move(self);  // self-assignment keeps the block
        CHECK(b.get() == pc && b.capacity() == 16 && Counting::frees == f0 + 1);
        CHECK(a.reserve(2) == 0 && a.capacity() == 2);  // a moved-from buffer is an empty one
    }
    CHECK(Counting::allocs == a0 + 3 && Counting::frees == f0 + 3 && Counting::live.empty());
}

void resets() {
    const int f0 = Counting::frees;
    {
        Buf b;
        b.reset();  // empty: nothing to free
        CHECK(Counting::frees == f0);
        CHECK(b.reserve(3) == 0);
        b.reset();
        CHECK(b.get() == nullptr && b.capacity() == 0 && Counting::frees == f0 + 1);
        b.reset();
        CHECK(Counting::frees == f0 + 1);
    }  // destruction after reset()
    CHECK(Counting::frees == f0 + 1);
    {
        Buf b;
        CHECK(b.reserve(3) == 0);
    }  // destruction alone frees
    CHECK(Counting::frees == f0 + 2);
}

}  // namespace

int main() {
    static_assert(!std::is_copy_constructible_v<Buf> && !std::is_copy_assignable_v<Buf>, "move-only");
    static_assert(std::is_nothrow_move_constructible_v<Buf> && std::is_nothrow_move_assignable_v<Buf>, "movable");
    reserve_rules();
    moves();
    resets();
    CHECK(Counting::allocs == Counting::frees && Counting::live.empty());
    std::printf("checks %d allocs %d frees %d\nok\n", g_checks, Counting::allocs, Counting::frees);
    return 0;
}
