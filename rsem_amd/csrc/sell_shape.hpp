// sell_shape.hpp -- the shape record of the sliced layout (sell_layout.hpp) and the index arithmetic from a sorted read to its
// place in the planes.  Included INSIDE an anonymous namespace by sell_layout.hpp (em.hip, gibbs.hip, the CPU emulators) and
// by model.hip, whose round kernel writes the alignment probabilities straight into the value planes.
#pragma once

// value plane formats (sell_layout.hpp).  F64X: doubles, rows that are only the IN-WINDOW part of a read whose other
// alignments live in the far-entry side arrays (split rows); such a row carries an extra term in its normaliser and hands
// its reciprocal on.
constexpr int kFmtF64 = 0, kFmtQ32 = 1, kFmtF64X = 2;
// Shapes a layout can hold (sell_layout.hpp: kMaxShapes): the kernels that keep the table in LDS size it by this.
constexpr int kShapeTableMax = 148;

struct Shape {
    uint64_t plane_base;  // first plane of this shape (one plane = 64 entries)
    uint32_t slice_base;  // first slice
    uint32_t n_slices;
    uint32_t row_base;    // first sorted row
    uint32_t n_rows;
    uint32_t slot_base;   // first row slot (slot = slice * rows_per_slice + r)
    int32_t K;            // planes per slice
    int32_t lg;           // log2(lanes per read)
    int32_t fmt;          // kFmtF64 / kFmtQ32
    uint64_t val_base;    // byte offset of this shape's value planes (512 B per F64 plane, 256 B per Q32 plane)
    int32_t cut;          // groups of 16 entries the LAST value plane of a slice is stored without, 0..3 (0: a full plane)
    int32_t reserved;     // (keeps the record free of padding bytes: units are compared byte by byte)
};

__host__ __device__ inline uint32_t plane_bytes(int fmt) { return fmt == kFmtQ32 ? 256u : 512u; }

__host__ __device__ inline int shape_G(const Shape& S) {  // lanes per read
    return 1 << S.lg;
}
__host__ __device__ inline uint32_t shape_R(const Shape& S) {  // reads per slice
    return 64u >> S.lg;
}

// ---- where a VALUE lives ------------------------------------------------------------------------------------------------
// Entry c of a read sits in plane c >> lg, lane r * G + (c & (G - 1)); every empty entry of a read with K >= 3 planes
// therefore sits in plane K - 1, in the read's lanes g >= L - (K - 1) * G.  A shape whose reads all leave the same quarters
// of their lane group empty there (cut = 4 - quarters used) stores that plane COMPACTED: Gk = G * (4 - cut) / 4 entries
// per read, side by side, 64 - 16 * cut per slice.  Planes 0 .. K-2 and all the sid planes keep their 64 entries.
// Everything that touches a value entry goes through these three functions.
__host__ __device__ inline uint32_t shape_val_stride(int K, int cut) {  // value entries per slice
    return (uint32_t)(K * 64 - 16 * cut);
}
__host__ __device__ inline uint32_t shape_val_stride(const Shape& S) { return shape_val_stride(S.K, S.cut); }
__host__ __device__ inline int shape_Gk(int lg, int cut) {  // lanes of a read that hold an entry in the last plane
    return ((1 << lg) * (4 - cut)) >> 2;
}
__host__ __device__ inline int shape_Gk(const Shape& S) { return shape_Gk(S.lg, S.cut); }
// alignment c of the read in row slot r -> entry within the slice's value planes; `ok` false: the shape has no such entry
// (cannot happen for a read that was given this shape by its length)
__host__ __device__ inline uint32_t shape_val_off(int lg, int K, int cut, uint32_t r, int c, bool* ok = nullptr) {
    const int k = c >> lg, g = c & ((1 << lg) - 1);
    if (k < K - 1 || cut == 0) {
        if (ok) *ok = k < K;
        return (uint32_t)k * 64u + (r << lg) + (uint32_t)g;
    }
    const int Gk = shape_Gk(lg, cut);
    if (ok) *ok = k == K - 1 && g < Gk;
    return (uint32_t)(K - 1) * 64u + r * (uint32_t)Gk + (uint32_t)g;
}
__host__ __device__ inline uint32_t shape_val_off(const Shape& S, uint32_t r, int c, bool* ok = nullptr) {
    return shape_val_off(S.lg, S.K, S.cut, r, c, ok);
}
__host__ __device__ inline uint64_t shape_val_bytes(const Shape& S) {  // all value planes of the shape
    return (uint64_t)S.n_slices * shape_val_stride(S) * (plane_bytes(S.fmt) / 64u);
}

// sorted read q of a shape  ->  (slice within the shape, row slot within the slice)
__host__ __device__ inline void row_to_slot(const Shape& S, uint32_t T, uint32_t q, uint32_t& slice_local, uint32_t& r) {
    const uint32_t R = shape_R(S), rpb = R * T;
    const uint32_t b = q / rpb, qb = q % rpb;
    const uint32_t left = S.n_rows - b * rpb;
    const uint32_t nb = left < rpb ? left : rpb;
    const uint32_t Tb = (nb + R - 1) / R;
    r = qb / Tb;
    slice_local = b * T + qb % Tb;
}

