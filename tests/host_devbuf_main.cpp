// csrc/ck_devbuf.h on a counting malloc policy whose next allocation can be made to fail, as a stand-alone program for
// -fsanitize=address,undefined (tests/test_devbuf_host.py).  Every check is a condition; a failed one exits with 1.
#include <stdio.h>
#include <stdlib.h>

#include "ck_devbuf.h"

struct Counting {
    static int live, takes, releases, fail_in;   // fail_in = k > 0: the k-th allocation from now fails
    static int take(void** p, size_t bytes) {
        if (fail_in > 0 && --fail_in == 0) return 2;
        *p = malloc(bytes ? bytes : 8);
        ++live, ++takes;
        return 0;
    }
    static void release(void* p) {
        free(p);
        --live, ++releases;
    }
};
int Counting::live = 0, Counting::takes = 0, Counting::releases = 0, Counting::fail_in = 0;

template <class T>
using Buf = DevBufOf<T, Counting>;
using Temps = DevTempsOf<Counting>;

#define CHECK(c)                                                     \
    do {                                                             \
        if (!(c)) {                                                  \
            printf("FAILED line %d: %s\n", __LINE__, #c);            \
            exit(1);                                                 \
        }                                                            \
    } while (0)

struct Group {   // a joint-lifetime group as the handle's Schur and variogram structs
    long long order = 0;
    std::vector<Buf<double>> panels;
    Buf<double> a, b;
    Buf<int> c;
};

// the shape of ensure_panels: build into locals, commit only when every allocation has succeeded
struct Panels {
    Buf<char> slab;
    Buf<double*> ptr;
    Buf<int> map;
};
static int build_panels(Panels& out) {
    Panels p;
    if (p.slab.reserve(4096)) return -1;
    if (p.ptr.reserve(8)) return -1;
    if (p.map.reserve(9)) return -1;
    out = std::move(p);
    return 0;
}

int main() {
    {
        Buf<double> b;
        CHECK(b.get() == nullptr && b.cap() == 0);
        CHECK(b.reserve(100) == 0 && b.cap() == 100 && Counting::live == 1);
        double* p = b;
        for (int i = 0; i < 100; ++i) p[i] = i;   // the sanitizer sees all 100 elements
        CHECK(b.reserve(40) == 0 && b.get() == p && b.cap() == 100);   // below the capacity: the pointer stays
        CHECK(b.reserve(100) == 0 && b.get() == p && Counting::takes == 1);
        const int rel = Counting::releases;
        CHECK(b.reserve(101) == 0 && b.cap() == 101 && Counting::releases == rel + 1 && Counting::live == 1);   // growth frees once
        b.get()[100] = 1.0;
        // a failed reserve leaves the buffer empty with capacity 0, and nothing live
        Counting::fail_in = 1;
        CHECK(b.reserve(1000) == 2 && b.get() == nullptr && b.cap() == 0 && Counting::live == 0);
        CHECK(b.reserve(10) == 0 && b.cap() == 10 && Counting::live == 1);   // ... and a retry allocates again
        // a request of 0 elements on an empty buffer still gets a pointer
        Buf<int> z;
        CHECK(z.reserve(0) == 0 && z.get() != nullptr && z.cap() == 0 && Counting::live == 2);
        // move assignment releases the target and empties the source
        Buf<double> c;
        CHECK(c.reserve(7) == 0 && Counting::live == 3);
        double* pb = b.get();
        c = std::move(b);
        CHECK(Counting::live == 2 && c.get() == pb && c.cap() == 10 && b.get() == nullptr && b.cap() == 0);
        Buf<double> d(std::move(c));
        CHECK(Counting::live == 2 && d.get() == pb && c.get() == nullptr && c.cap() == 0);
        // a view never releases, whatever happens to it
        const int rel2 = Counting::releases;
        {
            Buf<double> v, w;
            v.view(d.get() + 2, 8);
            CHECK(v.get() == pb + 2 && v.cap() == 8);
            w = std::move(v);
            w.reset();
            v.view(d.get(), 10);
            v.view(d.get() + 1, 9);   // a carve abandoned for another
        }
        CHECK(Counting::releases == rel2 && Counting::live == 2);
        // a view that grows becomes an owner; an owner that becomes a view releases
        Buf<double> g;
        g.view(d.get(), 10);
        CHECK(g.reserve(11) == 0 && Counting::live == 3 && g.get() != pb);
        g.view(d.get(), 10);
        CHECK(Counting::live == 2);
        d.get()[9] = 2.0;   // still alive
    }
    CHECK(Counting::live == 0);
    {   // a struct of buffers assigned {} releases all of them
        Group s;
        s.order = 1024;
        s.panels.resize(3);
        for (auto& p : s.panels) CHECK(p.reserve(64) == 0);
        CHECK(s.a.reserve(5) == 0 && s.b.reserve(6) == 0 && s.c.reserve(7) == 0 && Counting::live == 6);
        s = {};
        CHECK(Counting::live == 0 && s.order == 0 && s.panels.empty() && s.a.get() == nullptr && s.c.cap() == 0);
        CHECK(s.a.reserve(5) == 0);
    }
    CHECK(Counting::live == 0);
    {   // the temporaries of one call
        Temps t;
        double* x = nullptr;
        int* y = nullptr;
        char* e = nullptr;
        CHECK(t.get(&x, 80) == 0 && t.get(&y, 12) == 0 && t.get(&e, 0) == 0 && x && y && e && Counting::live == 3);
        x[9] = 1.0, y[2] = 3;
        Counting::fail_in = 1;
        CHECK(t.get(&x, 16) == 2 && x == nullptr && Counting::live == 3);
    }
    CHECK(Counting::live == 0);
    {   // three reserves, the second failing: nothing is taken, the target is untouched; then the commit
        Panels h;
        Counting::fail_in = 2;
        CHECK(build_panels(h) == -1 && Counting::live == 0 && h.slab.get() == nullptr && h.ptr.get() == nullptr && h.map.get() == nullptr);
        CHECK(build_panels(h) == 0 && Counting::live == 3 && h.slab.cap() == 4096 && h.ptr.cap() == 8 && h.map.cap() == 9);
        Counting::fail_in = 3;
        char* keep = h.slab;
        CHECK(build_panels(h) == -1 && Counting::live == 3 && h.slab.get() == keep);
    }
    CHECK(Counting::live == 0 && Counting::takes == Counting::releases);
    printf("all checks passed (%d allocations)\n", Counting::takes);
    return 0;
}
