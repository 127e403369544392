// TEST INFRASTRUCTURE (not product code): what the stand-alone sanitizer programs (tests/host_emul/*_asan_main.cpp) share — the pseudo-random inputs, heap
// buffers of EXACTLY their size, the test that a kernel wrote all of an output.  Shapes and case loops are each program's own.
#pragma once
#include <cstddef>

namespace {

struct Rng {
    unsigned long long s;
    unsigned next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (unsigned)(s >> 33); }
    float uniform() { return (float)(next() & 0xffffff) / (float)0x1000000; }
};

template <class T> struct Heap {                                     // operator new: 16-byte aligned, no slack behind the last element
    T* p; size_t n;
    explicit Heap(size_t n_) : p(new T[n_ ? n_ : 1]), n(n_) {}
    ~Heap() { delete[] p; }
    Heap(const Heap&) = delete;
};

inline bool finite_all(const float* p, size_t n)
{
    for (size_t i = 0; i < n; i++) if (!(p[i] - p[i] == 0.f)) return false;
    return true;
}
inline bool finite_all(const Heap<float>& h) { return finite_all(h.p, h.n); }

}  // namespace
