// One piece of scratch, many parts: the arithmetic every layout struct shares (op_layouts.h, train_layouts.h, icp_layout.h, icp_grid.h, cell_index.h
// and the layouts that live beside their kernels).  Plain C++ that compiles for the host too (tools/scratch_layout_check.cpp).
// A layout is built from an operator's shape alone, holds its parts' offsets and `bytes`, and is read by the size function and the
// launcher alike: the two cannot disagree.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace dsir {

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// parts in declaration order, each starting on 256 bytes: take() returns the part's offset, p is the size so far
struct Carve {
  size_t p = 0;
  size_t take(size_t bytes) { const size_t off = p; p += align256(bytes); return off; }
};

// the part at byte offset `off` of the piece at `base`
template <class T> inline T* at(void* base, size_t off) { return reinterpret_cast<T*>(static_cast<char*>(base) + off); }
template <class T> inline const T* at(const void* base, size_t off) { return reinterpret_cast<const T*>(static_cast<const char*>(base) + off); }

}  // namespace dsir
