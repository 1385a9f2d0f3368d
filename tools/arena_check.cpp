// Stand-alone host program around fgdm_amd/csrc/arena.h for a sanitizer run of the workspace allocator and its owning handles
// (no HIP, no Python: the slabs come from malloc):
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/arena_check.cpp -o arena_check && ./arena_check
#include "../fgdm_amd/csrc/arena.h"

#include <cstdio>
#include <cstdlib>
#include <utility>

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

static int slabs_made = 0, slabs_freed = 0;
static void* host_slab(size_t bytes) { ++slabs_made; return malloc(bytes); }
static void host_free(void* p) { ++slabs_freed; free(p); }

struct HostArena : Arena {
    explicit HostArena(size_t slab = 1 << 16) { slab_bytes = slab; slab_alloc = host_slab; slab_free = host_free; }
    size_t blocks() const { size_t n = 0; for (auto& s : slabs) n += s.size(); return n; }
    size_t free_blocks() const { size_t n = 0; for (auto& s : slabs) for (auto& b : s) n += b.free; return n; }
};
struct View { char* p = nullptr; int tag = 0; };      // stands in for the engine's Tensor
using Held = Owned<View>;
static Held take(Arena& a, size_t bytes, int tag = 0) { return Held(View{(char*)a.alloc(bytes), tag}, &a); }

// rounding, first fit, splitting
static void check_alloc() {
    HostArena a;
    char* p0 = (char*)a.alloc(1);          // 256
    char* p1 = (char*)a.alloc(257);        // 512
    char* p2 = (char*)a.alloc(0);          // 256
    EXPECT(p1 == p0 + 256 && p2 == p1 + 512);
    EXPECT(a.in_use == 1024 && a.peak == 1024 && a.reserved() == (1 << 16));
    EXPECT(a.blocks() == 4 && a.free_blocks() == 1);            // the split left the remainder free
    a.release(p1);
    EXPECT(a.in_use == 512 && a.free_blocks() == 2);
    char* q = (char*)a.alloc(300);                             // first fit: the 512-byte hole, which it fills whole
    EXPECT(q == p1 && a.blocks() == 4);
    a.release(q);
    char* r = (char*)a.alloc(200);                             // the hole again, split: 256 used, 256 stay free in place
    char* t = (char*)a.alloc(256);
    EXPECT(r == p1 && t == p1 + 256 && a.blocks() == 5);
    a.release(p0); a.release(p2); a.release(r); a.release(t);
    EXPECT(a.in_use == 0 && a.blocks() == 1 && a.peak == 1024);
    a.release(nullptr);
    a.release(p0);                                             // not handed out: nothing happens
    EXPECT(a.in_use == 0 && a.blocks() == 1);
}

// coalescing with the left neighbour, the right neighbour, and both
static void check_coalescing() {
    HostArena a;
    char* p[5];
    for (char*& q : p) q = (char*)a.alloc(256);
    EXPECT(a.blocks() == 6);
    a.release(p[0]); a.release(p[1]);                          // left neighbour free
    EXPECT(a.blocks() == 5 && a.free_blocks() == 2);
    a.release(p[4]);                                           // right neighbour free (the slab's tail)
    EXPECT(a.blocks() == 4 && a.free_blocks() == 2);
    a.release(p[3]);                                           // right again
    EXPECT(a.blocks() == 3 && a.free_blocks() == 2);
    a.release(p[2]);                                           // both
    EXPECT(a.blocks() == 1 && a.free_blocks() == 1 && a.in_use == 0);
    EXPECT((char*)a.alloc(1 << 16) == p[0]);                   // the slab is whole again
}

// a scripted sequence: in_use back at 0, the hand-computed peak, the same addresses when it runs again
static void script(HostArena& a, char* out[6]) {
    out[0] = (char*)a.alloc(1000);     // 1024                 in use 1024
    out[1] = (char*)a.alloc(5000);     // 5120                        6144
    out[2] = (char*)a.alloc(256);      //                             6400
    a.release(out[1]);                 //                             1280
    out[3] = (char*)a.alloc(2048);     // into the hole               3328
    out[4] = (char*)a.alloc(3072);     // the rest of the hole        6400
    out[5] = (char*)a.alloc(512);      // behind out[2]               6912   <- the peak
    a.release(out[0]); a.release(out[3]);
    a.release(out[5]); a.release(out[2]); a.release(out[4]);
}
static void check_script() {
    HostArena a;
    char *first[6], *second[6];
    script(a, first);
    EXPECT(a.in_use == 0 && a.peak == 6912 && a.blocks() == 1);
    EXPECT(first[3] == first[1] && first[4] == first[1] + 2048 && first[5] == first[2] + 256);
    script(a, second);
    for (int i = 0; i < 6; ++i) EXPECT(first[i] == second[i]);
    EXPECT(a.in_use == 0 && a.peak == 6912 && a.reserved() == (1 << 16));
}

// a request larger than the slab gets a slab of its own; a source without memory gives nullptr and changes nothing
static void check_slabs() {
    const int made0 = slabs_made, freed0 = slabs_freed;
    {
        HostArena a(4096);
        char* small = (char*)a.alloc(256);
        char* big = (char*)a.alloc(10000);                     // 10240 > 4096
        EXPECT(small && big && slabs_made == made0 + 2 && a.slabs.size() == 2);
        EXPECT(a.slabs[1].size() == 1 && a.slabs[1][0].sz == 10240 && a.reserved() == 4096 + 10240);
        char* more = (char*)a.alloc(4096);                     // fits neither remainder: a third slab
        EXPECT(more && a.slabs.size() == 3);
        a.release(big);
        EXPECT((char*)a.alloc(8192) == big);                   // slab order: the second slab serves it, split
        a.slab_alloc = [](size_t) -> void* { return nullptr; };
        const size_t in_use = a.in_use, peak = a.peak;
        EXPECT(a.alloc(1 << 20) == nullptr && a.in_use == in_use && a.peak == peak && a.slabs.size() == 3);
    }
    EXPECT(slabs_freed == freed0 + 3);                         // the arena gives its slabs back
}

// the handles: one release on destruction, on reset() and on move-assignment over a live handle; none from a moved-from one
static void check_handles() {
    HostArena a;
    {
        Held h = take(a, 256, 7);
        EXPECT(h.p && h.tag == 7 && h.from == &a && a.in_use == 256);
    }
    EXPECT(a.in_use == 0);
    Held h = take(a, 512);
    h.reset();
    EXPECT(a.in_use == 0 && !h.p && !h.from);
    h.reset();                                                 // again: nothing
    EXPECT(a.in_use == 0);
    {
        Held x = take(a, 256, 1), y = take(a, 1024, 2);
        char* yp = y.p;
        x = std::move(y);                                      // x's block goes back, y's moves in
        EXPECT(a.in_use == 1024 && x.p == yp && x.tag == 2 && !y.p && !y.from);
        Held z(std::move(x));
        EXPECT(a.in_use == 1024 && z.p == yp && !x.p && !x.from);
        x.reset();                                             // moved-from handles release nothing ...
        y.reset();
        EXPECT(a.in_use == 1024);
        Held& zr = z;
        z = std::move(zr);                                     // self-assignment keeps the block
        EXPECT(a.in_use == 1024 && z.p == yp);
    }                                                          // ... nor do their destructors: one release, of z
    EXPECT(a.in_use == 0 && a.blocks() == 1);
    {
        View elsewhere{(char*)&a, 3};
        Held v(elsewhere, nullptr);                            // a view: owns nothing
        Held empty;
        empty = std::move(v);
    }
    EXPECT(a.in_use == 0);
    {
        Buf raw(Raw{a.alloc(100)}, &a);
        EXPECT(raw.as<float>() == (float*)raw.p && a.in_use == 256);
    }
    EXPECT(a.in_use == 0);
    {                                                          // a failed allocation in a handle
        a.slab_alloc = [](size_t) -> void* { return nullptr; };
        Held none = take(a, 1 << 20);
        EXPECT(!none.p && a.in_use == 0);
    }
    EXPECT(a.in_use == 0);
}

// a handle goes back to the arena it came from, whichever arena is "current" by then
static void check_two_arenas() {
    HostArena A, B;
    Arena* current = &A;
    Held fromA = take(*current, 256);
    current = &B;
    Held fromB = take(*current, 512);
    EXPECT(A.in_use == 256 && B.in_use == 512);
    {
        Held moved = std::move(fromA);
        EXPECT(moved.from == &A);
    }                                                          // destroyed while B is current
    EXPECT(A.in_use == 0 && B.in_use == 512 && current == &B);
    fromB = take(A, 1024);                                     // B's block back to B, A's block in
    EXPECT(A.in_use == 1024 && B.in_use == 0 && fromB.from == &A);
    fromB.reset();
    EXPECT(A.in_use == 0 && A.blocks() == 1 && B.blocks() == 1);
}

int main() {
    check_alloc();
    check_coalescing();
    check_script();
    check_slabs();
    check_handles();
    check_two_arenas();
    EXPECT(slabs_made == slabs_freed);
    printf(failures ? "arena_check: %d FAILED\n" : "arena_check: all cases passed\n", failures);
    return failures ? 1 : 0;
}
