// Activation workspace of the engine: a first-fit free-list allocator over large slabs, and the move-only handles that own its
// blocks.  ONE RULE: whoever holds the handle owns the block; destruction, reset() and move-assignment over a live handle give it
// back to the arena it came from.  Nothing else releases.  No HIP in here unless the including file is HIP (tools/arena_check.cpp
// runs the whole header on the host over malloc'ed slabs).
#pragma once
#include <algorithm>
#include <cstddef>
#include <vector>

#ifdef __HIP__
#include <hip/hip_runtime.h>
static void* arena_device_slab(size_t bytes) { void* p = nullptr; return hipMalloc(&p, bytes) == hipSuccess ? p : nullptr; }
static void arena_device_free(void* p) { (void)hipFree(p); }
#else
static void* (*const arena_device_slab)(size_t) = nullptr;      // a host build names its own slab source
static void (*const arena_device_free)(void*) = nullptr;
#endif

// First-fit free-list allocator over slabs of device memory.  The allocation sequence of a forward pass is deterministic, so
// buffers land at the same addresses every call (graph-capture friendly) and recently freed (cache-hot) blocks are reused first.
struct Arena {
    struct Blk { char* p; size_t sz; bool free; };
    std::vector<std::vector<Blk>> slabs;
    std::vector<char*> bases;
    size_t slab_bytes = (size_t)4 << 30;
    size_t in_use = 0, peak = 0;
    void* (*slab_alloc)(size_t) = arena_device_slab;      // nullptr when it has no memory
    void (*slab_free)(void*) = arena_device_free;

    Arena() = default;
    Arena(const Arena&) = delete;
    ~Arena() { for (char* b : bases) slab_free(b); }
    void* alloc(size_t bytes) {
        bytes = (bytes + 255) & ~(size_t)255;
        if (bytes == 0) bytes = 256;
        for (auto& s : slabs)
            for (size_t i = 0; i < s.size(); ++i)
                if (s[i].free && s[i].sz >= bytes) {
                    if (s[i].sz > bytes) {
                        Blk rest{s[i].p + bytes, s[i].sz - bytes, true};
                        s[i].sz = bytes;
                        s.insert(s.begin() + i + 1, rest);
                    }
                    s[i].free = false;
                    in_use += bytes;
                    peak = std::max(peak, in_use);
                    return s[i].p;
                }
        const size_t sz = std::max(slab_bytes, bytes);
        char* base = (char*)slab_alloc(sz);
        if (!base) return nullptr;
        bases.push_back(base);
        slabs.push_back({Blk{base, sz, true}});
        return alloc(bytes);
    }
    void release(void* p) {
        if (!p) return;
        for (auto& s : slabs)
            for (size_t i = 0; i < s.size(); ++i)
                if (s[i].p == p && !s[i].free) {
                    s[i].free = true;
                    in_use -= s[i].sz;
                    if (i + 1 < s.size() && s[i + 1].free) { s[i].sz += s[i + 1].sz; s.erase(s.begin() + i + 1); }
                    if (i > 0 && s[i - 1].free) { s[i - 1].sz += s[i].sz; s.erase(s.begin() + i); }
                    return;
                }
    }
    size_t reserved() const { size_t r = 0; for (auto& s : slabs) for (auto& b : s) r += b.sz; return r; }
};

// The owning handle: a View (a plain struct with a pointer member `p`, such as the engine's Tensor) plus the arena that served
// `p`.  Move-only.  The block goes back to `from` -- the arena recorded here, whichever arena the engine is allocating from by
// then.  from == nullptr: a view of memory that is owned elsewhere (a persistent cache, another handle); it releases nothing.
template <class View> struct Owned : View {
    Arena* from = nullptr;
    Owned() = default;
    Owned(const View& v, Arena* a) : View(v), from(a) {}
    Owned(Owned&& o) noexcept : View(o), from(o.from) { o.p = nullptr; o.from = nullptr; }
    Owned& operator=(Owned&& o) noexcept {
        if (this != &o) { reset(); View::operator=(o); from = o.from; o.p = nullptr; o.from = nullptr; }
        return *this;
    }
    Owned(const Owned&) = delete;
    Owned& operator=(const Owned&) = delete;
    ~Owned() { reset(); }
    void reset() {      // release early; the shape fields of the view stay as they were
        if (from) from->release(this->p);
        this->p = nullptr;
        from = nullptr;
    }
};

// raw scratch: fp32 streams, statistics, split-K partials, the sampler loops' planes
struct Raw {
    void* p = nullptr;
    template <class T> T* as() const { return (T*)p; }
};
using Buf = Owned<Raw>;
