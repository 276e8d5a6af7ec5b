// scratch_layout_check.cpp -- csrc/scratch_layout.h on the host, under AddressSanitizer and UBSan (tests/test_host_logic.py builds and
// runs it).  The buffer is a malloc-backed stand-in for DevBuf: p, cap and a grow-only ensure that allocates EXACTLY what was asked, so
// that a slot one byte past the layout's total is a heap overflow the sanitizer reports.
#include "scratch_layout.h"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

struct HostBuf {
    void* p = nullptr;
    size_t cap = 0;
    void ensure(size_t n)
    {
        if (n <= cap) return;
        free(p);
        p = malloc(n);
        cap = n;
    }
    ~HostBuf() { free(p); }
};

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

struct Piece { size_t off, bytes, align; };
struct Rec20 { float score; int32_t a, b, c, d; };          // a 20-byte record (the detector's candidates are one)

struct Mixed {
    ScratchLayout lay;
    ScratchSlot<double> d; ScratchSlot<int32_t> i; ScratchSlot<uint8_t> b; ScratchSlot<Rec20> r; ScratchSlot<uint16_t> h; ScratchSlot<double> z;
    std::vector<Piece> pieces;
};
// every alignment with every kind of count (0, 1, odd, a multiple of the alignment) somewhere
static Mixed mixed(size_t n, size_t a0, size_t a1, size_t a2)
{
    Mixed m;
    m.d = m.lay.take<double>(n, a0);      m.pieces.push_back({m.d.off, m.d.bytes(), a0});
    m.i = m.lay.take<int32_t>(1, a1);     m.pieces.push_back({m.i.off, m.i.bytes(), a1});
    m.b = m.lay.take<uint8_t>(3 * n + 1, a2); m.pieces.push_back({m.b.off, m.b.bytes(), a2});
    m.z = m.lay.take<double>(0, a0);      m.pieces.push_back({m.z.off, m.z.bytes(), a0});
    m.r = m.lay.take<Rec20>(n + 7, a1);   m.pieces.push_back({m.r.off, m.r.bytes(), a1});
    m.h = m.lay.take<uint16_t>(64, a2);   m.pieces.push_back({m.h.off, m.h.bytes(), a2});
    return m;
}

template <class T>
static void touch(const ScratchSlot<T>& s, HostBuf& buf)
{
    T* p = s.in(buf);
    CHECK(reinterpret_cast<unsigned char*>(p) == static_cast<unsigned char*>(buf.p) + s.off);
    if (s.count == 0) return;
    unsigned char* q = reinterpret_cast<unsigned char*>(p);
    q[0] = 1; q[s.bytes() - 1] = 2;                          // first and last byte: clean under the sanitizers after ensure(bytes())
}

template <class F>
static bool throws(F f)
{
    try { f(); } catch (const PvfError&) { return true; }
    return false;
}

int main()
{
    const size_t aligns[3] = {16, 64, 256}, counts[] = {0, 1, 5, 64, 1000};
    for (size_t n : counts)
        for (int r = 0; r < 3; ++r) {
            const size_t a0 = aligns[r], a1 = aligns[(r + 1) % 3], a2 = aligns[(r + 2) % 3];
            Mixed m = mixed(n, a0, a1, a2);
            for (size_t k = 0; k < m.pieces.size(); ++k) {
                const Piece& p = m.pieces[k];
                CHECK(p.off % p.align == 0);
                CHECK(p.off + p.bytes <= m.lay.bytes());
                for (size_t j = 0; j < k; ++j) {             // pairwise disjoint (an empty slot overlaps nothing)
                    const Piece& o = m.pieces[j];
                    CHECK(p.bytes == 0 || o.bytes == 0 || p.off >= o.off + o.bytes || o.off >= p.off + p.bytes);
                }
            }
            // built twice from the same arguments: the same offsets and the same total
            const Mixed again = mixed(n, a0, a1, a2);
            CHECK(again.lay.bytes() == m.lay.bytes());
            for (size_t k = 0; k < m.pieces.size(); ++k) CHECK(again.pieces[k].off == m.pieces[k].off && again.pieces[k].bytes == m.pieces[k].bytes);
            // pad grows the total by what was asked and moves no slot
            const size_t before = m.lay.bytes();
            m.lay.pad(4096 + 1);
            CHECK(m.lay.bytes() == before + 4097);
            m.lay.pad(0);
            CHECK(m.lay.bytes() == before + 4097);
            // in(): refused on a buffer that was never ensured and on one ensured one byte short of the last slot's end
            HostBuf never, small, exact;
            CHECK(throws([&] { m.h.in(never); }));
            CHECK(throws([&] { m.i.in(never); }));
            small.ensure(m.h.off + m.h.bytes() - 1);
            CHECK(throws([&] { m.h.in(small); }));
            CHECK(!throws([&] { m.r.in(small); }));          // (the slots in front of it still fit)
            // every slot's first and last byte inside a buffer of exactly bytes() (pad taken back: the last slot ends the allocation)
            exact.ensure(before);
            touch(m.d, exact); touch(m.i, exact); touch(m.b, exact); touch(m.z, exact); touch(m.r, exact); touch(m.h, exact);
        }
    // an empty layout, and an empty slot at the very end of an exact buffer
    ScratchLayout e;
    CHECK(e.bytes() == 0);
    const auto one = e.take<int32_t>(1, 16);
    const auto none = e.take<double>(0, 16);
    CHECK(e.bytes() == 16 && none.off == 16 && none.bytes() == 0);
    HostBuf b16;
    b16.ensure(e.bytes());
    touch(one, b16); touch(none, b16);
    printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
