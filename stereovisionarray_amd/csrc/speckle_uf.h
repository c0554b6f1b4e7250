// speckle_uf.h -- lock-free union-find on a label plane (label equivalence),
// as templates over a small memory policy, shared by speckle.hip (LDS and
// global-memory policies on atomics) and the host test programs (plain-memory
// policies; tests/test_speckle_cpu.py).  Plain C++: no HIP header.
//
// A policy M gives
//   uint32_t load(uint32_t i)                    -- the label of element i
//   uint32_t min_exchange(uint32_t i, uint32_t v) -- label[i] = min(label[i], v),
//                                                   atomically; returns the old value
//
// Invariants:
//   * label[i] <= i always: an element is a root iff label[i] == i, and the
//     root of a finished component is its smallest index;
//   * labels only decrease (min_exchange is the only write);
//   * no thread ever waits for another thread's progress: there is no lock, no
//     spin-wait and no flag, and the only ordering between passes is the launch
//     boundary;
//   * every loop ends because a value strictly decreases: find's index, and in
//     unite the larger of (a, b).
//
// load may return ANY EARLIER value of the word (a plain load of a word that
// another XCD's atomics modify in the same launch can be stale; so can a relaxed
// atomic one, by a little).  Every earlier value of label[i] is <= i and lies in
// i's component, so find still ends at an element of that component that was
// once a root, and unite stays right because the decision is taken by
// min_exchange on the true value: if a was no longer a root, old != a, and the
// loop goes on with (old, b) -- the link a -> old that the minimum may have
// replaced is re-made through old.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SVA_UF_HD __host__ __device__
#else
#define SVA_UF_HD
#endif

namespace sva {
namespace uf {

// The root of i as far as load shows it.  Ends: the index strictly decreases.
template <class M>
SVA_UF_HD inline uint32_t find(M& m, uint32_t i) {
    uint32_t p = m.load(i);
    while (p < i) {
        i = p;
        p = m.load(i);
    }
    return i;
}

// Join the components of a and b.  Ends: max(a, b) strictly decreases.
template <class M>
SVA_UF_HD inline void unite(M& m, uint32_t a, uint32_t b) {
    a = find(m, a);
    b = find(m, b);
    while (a != b) {
        if (a < b) {
            const uint32_t t = a;
            a = b;
            b = t;
        }
        const uint32_t old = m.min_exchange(a, b);
        if (old == a) break;   // a was a root and now points at b
        a = old;               // a had a parent already: join that with b
    }
}

}  // namespace uf
}  // namespace sva
