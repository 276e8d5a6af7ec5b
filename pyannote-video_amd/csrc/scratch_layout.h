// scratch_layout.h -- how one grow-only buffer is shared out among several arrays (no HIP here: a host-only program can include it).
//
//     ScratchLayout lay;
//     auto a = lay.take<double>(n);           // offsets only, nothing is allocated
//     auto b = lay.take<int>(m, 64);
//     lay.pad(256);                           // a named tail, with a comment that says who reads or writes past the last array
//     buf.ensure(lay.bytes());                // ONE ensure per buffer per call: the carved total and the ensured size are one number
//     double* pa = a.in(buf);                 // refused if the slot does not lie inside the buffer
//
// A slot starts on a multiple of `align` and occupies its size rounded up to `align`, so slots never share an `align` unit and a
// layout built twice from the same arguments gives the same offsets.
#pragma once
#include <cstddef>
#include <stdexcept>

struct PvfError : std::runtime_error { using std::runtime_error::runtime_error; };

template <class T>
struct ScratchSlot {
    size_t off = 0, count = 0;
    size_t bytes() const { return count * sizeof(T); }
    // Buf: anything with `p` and `cap` (DevBuf, HostBuf)
    template <class Buf>
    T* in(const Buf& b) const
    {
        if (off + bytes() > b.cap) throw PvfError("scratch layout: a slot ends past its buffer (carved before ensure, or from another buffer)");
        return reinterpret_cast<T*>(static_cast<unsigned char*>(b.p) + off);
    }
};

struct ScratchLayout {
    size_t end = 0;
    static size_t up(size_t v, size_t align) { return (v + align - 1) / align * align; }
    template <class T>
    ScratchSlot<T> take(size_t count, size_t align = 256)
    {
        ScratchSlot<T> s;
        s.off = up(end, align); s.count = count;
        end = s.off + up(s.bytes(), align);
        return s;
    }
    void pad(size_t bytes) { end += bytes; }
    size_t bytes() const { return end; }
};
