// ck_devbuf.h -- ownership of device memory: DevBuf (one buffer that lives with its owner) and DevTemps (the temporaries
// of one call).  The allocation policy is a template parameter only so that tests/host_devbuf_main.cpp can run both on malloc.
#pragma once
#include <stddef.h>

#include <utility>
#include <vector>

// Move-only owner of n elements of device memory, or a non-owning window (view) into memory someone else owns -- a carve of
// the handle's arena.  Converts to T*, so launches and copies take it where they took the raw pointer.
template <class T, class P>
class DevBufOf {
    T* p_ = nullptr;
    size_t cap_ = 0;
    bool owns_ = false;

public:
    using err_t = decltype(P::take((void**)nullptr, (size_t)0));
    DevBufOf() = default;
    DevBufOf(DevBufOf&& o) noexcept : p_(o.p_), cap_(o.cap_), owns_(o.owns_) { o.p_ = nullptr, o.cap_ = 0, o.owns_ = false; }
    DevBufOf& operator=(DevBufOf&& o) noexcept {
        if (this != &o) {
            reset();
            p_ = o.p_, cap_ = o.cap_, owns_ = o.owns_;
            o.p_ = nullptr, o.cap_ = 0, o.owns_ = false;
        }
        return *this;
    }
    ~DevBufOf() { reset(); }
    void reset() {
        if (owns_ && p_) P::release(p_);
        p_ = nullptr, cap_ = 0, owns_ = false;
    }
    // room for n elements; grow-only, the contents are not kept (released before the larger block is taken).  On failure the
    // buffer is empty with capacity 0
    err_t reserve(size_t n) {
        if (p_ && n <= cap_) return err_t{};
        reset();
        const err_t e = P::take((void**)&p_, n * sizeof(T));
        if (e != err_t{}) {
            p_ = nullptr;
            return e;
        }
        cap_ = n, owns_ = true;
        return e;
    }
    void view(T* p, size_t n) {
        reset();
        p_ = p, cap_ = n;
    }
    T* get() const { return p_; }
    size_t cap() const { return cap_; }
    operator T*() const { return p_; }
};

// device temporaries of one call: released on every return path
template <class P>
struct DevTempsOf {
    std::vector<DevBufOf<char, P>> p;
    template <class T>
    typename DevBufOf<char, P>::err_t get(T** out, size_t bytes) {
        DevBufOf<char, P> b;
        const auto e = b.reserve(bytes);
        *out = (T*)b.get();
        if (b.get()) p.push_back(std::move(b));
        return e;
    }
};

#ifdef __HIP__   // the product policy; a request of 0 bytes still gets a pointer of its own
struct HipAlloc {
    static hipError_t take(void** p, size_t bytes) { return hipMalloc(p, bytes ? bytes : 8); }
    static void release(void* p) { (void)hipFree(p); }
};
template <class T>
using DevBuf = DevBufOf<T, HipAlloc>;
using DevTemps = DevTempsOf<HipAlloc>;
#endif
