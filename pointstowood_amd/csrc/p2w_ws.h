// The caller-allocated workspace of an entry point, described once.  Every workspace has ONE carve function that takes an
// arena and the size arguments and returns typed pointers (plus the counts derived from the sizes); p2w_*_ws_bytes() runs it
// on a null-based arena and returns bytes(), the launcher runs it on the real workspace and uses the pointers - so the size
// an entry point asks for and the memory it touches cannot drift apart.  Host code only.
#pragma once
#include <stddef.h>

struct P2wArena {
    explicit P2wArena(void* ws = nullptr) : base(static_cast<char*>(ws)) {}       // nullptr: only measure

    static size_t up(size_t v, size_t align = 256) { return (v + align - 1) & ~(align - 1); }   // align: a power of two

    // `count` elements of T at the current offset (nullptr on a null base); the offset advances by their size rounded up to `align`
    template <typename T> T* take(size_t count, size_t align = 256) { return static_cast<T*>(at(count * sizeof(T), align, alignof(T))); }
    // `n` raw bytes: a nested sub-workspace (carved by its own function from the returned pointer), or explicit slack
    void* raw(size_t n, size_t align = 256) { return at(n, align, 1); }
    size_t bytes() const { return off; }

private:
    char* base;
    size_t off = 0;
    void* at(size_t n, size_t align, size_t type_align) {
        void* p = base ? base + off : nullptr;                 // no arithmetic on a null base
#ifdef P2W_WS_TRACE                                            // tools/ws_layout_check.cpp records every region through this
        P2W_WS_TRACE(p, n, type_align);
#endif
        (void)type_align;
        off += up(n, align);
        return p;
    }
};

// what a carve function takes: p2w_ws_bytes([&](P2wArena& a) { x_carve(a, n); })
template <class Carve> static inline size_t p2w_ws_bytes(Carve carve) { P2wArena a; carve(a); return a.bytes(); }
