// snmf_host64.h -- small host helpers the fp64 units share (snmf_tu_solve64.hip, snmf_tu_train64.hip, snmf_tu_batch64.hip).
// Host code only, and nothing of the kernels' headers: a unit that includes this gets no kernel with it.
#pragma once
#include <stddef.h>

#include <algorithm>

// workgroups of 256 threads of an element-wise pass over n elements (the kernels stride over the grid beyond 8192)
inline int grid64(long long n) { return (int)std::max<long long>(1, std::min<long long>((n + 255) / 256, 8192)); }

// splits of a contraction of length K cut into pieces of `chunk` indices (kS64ChunkK of snmf_solve64.h)
inline int n_splits(int K, int chunk) { return (K + chunk - 1) / chunk; }

// Doubles of split partials an M x N product contracted over K needs: one M x N partial per split when it is split at all,
// none when its one split stores straight into the result.  The products of a solve run one after the other and share the
// partials, so a workspace takes the largest of these over its products.
inline size_t split_partials(size_t M, size_t N, int K, int chunk) {
    const int nz = n_splits(K, chunk);
    return nz > 1 ? (size_t)nz * M * N : 0;
}

// Pieces of one device block, 256-byte aligned, handed out in the order they are asked for.  base == nullptr only measures:
// the same walk gives the size to allocate.
struct Carve64 {
    char* base;
    size_t off = 0;
    explicit Carve64(void* b) : base((char*)b) {}
    template <typename E>
    E* get(size_t n) {
        E* q = base ? (E*)(base + off) : nullptr;
        off += (std::max<size_t>(n, 1) * sizeof(E) + 255) & ~(size_t)255;
        return q;
    }
};
