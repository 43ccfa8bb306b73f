// Stand-alone check of fvgp_amd/csrc/carve.h (built with -fsanitize=address,undefined by tests/test_carve_host.py): a layout walked over
// a null base and over a malloc of exactly bytes() gives the same offsets and total for mixed types and alignments, the pieces are
// disjoint and inside the buffer (their first and last bytes are written: the sanitizer sees an overrun), nested layouts compose, and a
// sub-view is the piece's own memory.
#include "carve.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {

int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

struct Piece { int64_t at, bytes, align; };
struct State { double a[3]; long long b; int c[5]; };          // 56 bytes: no multiple of 16

// every piece a walk hands out, as offsets from the base (measure mode: from the running total, which take() defines)
struct Walk {
    Carve &c;
    std::vector<Piece> pieces;
    template <class T>
    T *take(int64_t count, int64_t align) {
        const int64_t at = Carve::round_up(c.bytes(), align);
        T *p = c.take<T>(count, align);
        if (c.base) CHECK(reinterpret_cast<char *>(p) == c.base + at);
        else CHECK(p == nullptr);
        CHECK(c.bytes() == Carve::round_up(at + count * (int64_t)sizeof(T), align));
        pieces.push_back({at, count * (int64_t)sizeof(T), align});
        return p;
    }
};

// an inner layout, as pivot_layout sits inside sel_layout: it goes on where the outer one stands
struct Inner { double *slot; State *st; unsigned char *flags; };
Inner inner_layout(Walk &w, int64_t n) {
    Inner l;
    l.slot = w.take<double>(3, 16);
    l.st = w.take<State>(1, 16);
    l.flags = w.take<unsigned char>(n, 16);
    return l;
}

struct Outer { double *vec; Inner in; int *packed; double *tail, *tail_view; long *words; int *last; };
Outer outer_layout(Walk &w, int64_t n) {
    Outer l;
    l.vec = w.take<double>(n, 16);
    l.in = inner_layout(w, n);
    l.packed = w.take<int>(n, sizeof(int));                    // may end off an 8-byte boundary
    l.tail = w.take<double>(2 * n + 1, sizeof(double));        // packed doubles: the start is rounded up to 8
    l.tail_view = w.c.view<double>(l.tail, n);
    l.words = w.take<long>(n, 16);
    l.last = w.take<int>(n, sizeof(int));
    return l;
}

void run(int64_t n) {
    Carve m;
    Walk wm{m, {}};
    const Outer om = outer_layout(wm, n);
    CHECK(om.vec == nullptr && om.tail_view == nullptr && om.in.st == nullptr);
    const int64_t total = m.bytes();

    char *buf = static_cast<char *>(std::malloc((size_t)total));
    Carve c(buf);
    Walk wc{c, {}};
    const Outer oc = outer_layout(wc, n);
    CHECK(c.bytes() == total);
    CHECK(wc.pieces.size() == wm.pieces.size());
    for (size_t i = 0; i < wc.pieces.size(); ++i) {
        const Piece &p = wc.pieces[i], &q = wm.pieces[i];
        CHECK(p.at == q.at && p.bytes == q.bytes);
        CHECK(p.at % p.align == 0);
        CHECK(p.at >= 0 && p.at + p.bytes <= total);
        if (i) CHECK(wc.pieces[i - 1].at + wc.pieces[i - 1].bytes <= p.at);      // in order and disjoint
        if (p.bytes) { buf[p.at] = (char)i; buf[p.at + p.bytes - 1] = (char)i; } // first and last byte, inside the malloc
    }
    for (size_t i = 0; i < wc.pieces.size(); ++i) {                              // nobody wrote over anybody's ends
        const Piece &p = wc.pieces[i];
        if (p.bytes) CHECK(buf[p.at] == (char)i && buf[p.at + p.bytes - 1] == (char)i);
    }
    // typed use of every piece, end to end
    for (int64_t i = 0; i < n; ++i) { oc.vec[i] = 1.0; oc.in.flags[i] = 1; oc.packed[i] = 2; oc.words[i] = 3; oc.last[i] = 4; }
    for (int64_t i = 0; i < 2 * n + 1; ++i) oc.tail[i] = 5.0;
    oc.in.slot[2] = 6.0; oc.in.st->b = 7; oc.in.st->c[4] = 8;
    CHECK(oc.tail_view == oc.tail + n);
    oc.tail_view[n] = 9.0;                                                      // the view's last element is the piece's last
    CHECK(oc.tail[2 * n] == 9.0);
    CHECK(reinterpret_cast<char *>(oc.last + n) == buf + total);                // the last piece ends where bytes() says
    std::free(buf);
}

}  // namespace

int main() {
    // an empty walk, and a count of zero, take nothing
    Carve e;
    CHECK(e.bytes() == 0);
    CHECK(e.take<double>(0, 16) == nullptr && e.bytes() == 0);
    // 16 rounds both ends, sizeof packs
    Carve a;
    a.take<double>(3, 16); CHECK(a.bytes() == 32);
    a.take<int>(3, sizeof(int)); CHECK(a.bytes() == 44);
    a.take<double>(1, sizeof(double)); CHECK(a.bytes() == 56);
    a.take<char>(1, 16); CHECK(a.bytes() == 80);
    for (int64_t n : {1, 2, 3, 7, 8, 15, 16, 17, 129, 1000}) run(n);
    if (failures) { std::printf("%d check(s) failed\n", failures); return 1; }
    std::printf("carve ok\n");
    return 0;
}
