// One walk over a workspace, for its size query and for its entry point alike.  A layout function takes a Carve and calls take() once
// per piece, in order; over a null base the walk only counts (the query returns bytes()), over the caller's pointer the same calls
// hand out the typed pieces (the entry compares bytes() with what it was given).  Plain C++17, no HIP.
#pragma once
#include <cstdint>

struct Carve {
    char *base;               // nullptr: measure only
    int64_t used = 0;         // bytes handed out so far, padding included

    explicit Carve(void *work = nullptr) : base(static_cast<char *>(work)) {}

    // `count` objects of T in a piece that begins and ends on a multiple of `align` bytes (a power of two, >= alignof(T)) from the base:
    // 16 keeps every later offset 16-byte aligned (what even_up did for pieces counted in doubles), sizeof(T) packs
    template <class T>
    T *take(int64_t count, int64_t align = 16) {
        const int64_t at = round_up(used, align);
        used = round_up(at + count * (int64_t)sizeof(T), align);
        return base ? reinterpret_cast<T *>(base + at) : nullptr;
    }
    // a deliberate alias: the part of `piece` from element `index` on, under its own name and type (offset in units of T; 8- or
    // 16-byte pieces only ever hand out aligned views)
    template <class T, class U>
    T *view(U *piece, int64_t index = 0) const {
        return base ? reinterpret_cast<T *>(piece) + index : nullptr;
    }
    int64_t bytes() const { return used; }

    static int64_t round_up(int64_t v, int64_t align) { return (v + align - 1) & ~(align - 1); }
};

// what a size query returns: the layout function walked in measure mode at the entry's size arguments
template <class F, class... A>
int64_t carve_bytes(F layout, A &&...args) {
    Carve c;
    layout(c, args...);
    return c.bytes();
}
// the same for a layout function that hands its pointers to a struct of the entry's own (its kernel arguments) as the last argument
template <class T, class F, class... A>
int64_t carve_bytes_for(F layout, A &&...args) {
    T out{};
    return carve_bytes(layout, args..., out);
}
