// The Brakedown linear code (poly-commit/src/linear_codes/brakedown.rs, multilinear_brakedown/mod.rs:56-122) over the scalar fields:
// a batched sparse vector-matrix product (SprsMat::row_mul, linear_codes/utils.rs:41-52, applied to every row of the coefficient
// matrix), the base code (naive_reed_solomon, multilinear_brakedown/mod.rs:111-122) and the schedule of one encode.
//
// Mapping: lanes over the ROWS of the coefficient matrix, on a transposed working buffer T[position][row] (32-byte elements).  Lane g
// owns output (g / rows, g % rows).  From 64 rows on, the lanes of a wave share one output column: they all use the same (col_ind, val)
// entry -- one address, served as a broadcast --, their loop lengths are equal (no divergence on the ragged column lengths), and their
// 32-byte element loads are contiguous (rows x 32 bytes per entry).  With fewer than 64 rows a wave packs 64 / rows DIFFERENT columns,
// whose loop lengths and entry addresses differ (2 rows: in effect one lane per output element); those sizes are bound by launch
// latency, not by this (profiles/EXPERIMENTS.md 000).  The messages enter and the codewords leave row-major (the layout of the rest of
// the ABI): one transpose in, one out, 128 contiguous bytes per lane and step.
//
// The reference's loop order is kept, not repaired.  The last loop of encode (mod.rs:79-82) runs level 0 FIRST
// (`start.iter().zip(&end).enumerate()`, no `.rev()`), and cw[start[0]..end[0]] covers the places the later levels write: level i
// reads zeros wherever a level j > i has not written yet, and no B product reads another B product's output.  So every B product
// depends only on the A chain and the base code; all of them run as ONE launch, each clipped to the entries whose input position is
// below end[last] (what lies above is still zero when the reference's level i runs).  The commitment is defined by this order.
//
// Field addition is exact, so the order of summation is free: products are taken in pairs with one Montgomery reduction per pair
// (mul_add_mul) and every stored element is a canonical residue (the column hash absorbs the bytes).  The lazy (_lz) forms of fp32.hpp
// need spare top bits that none of the three scalar fields it was built for has (R >= 8p for the fused pair: none; 4p within the limbs: BN254 Fr only;
// BLS12-377's 253-bit Fr has both and runs the same canonical forms).  Each output has one owner: no
// atomics.  Everything is PC_HD and templated on the backend, so tests/emu steps the same bodies lane by lane on the CPU.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <vector>
#include "fp32.hpp"

namespace pc {

static constexpr uint32_t SPRS_MAX_LEVELS = 16;      // the default parameters reach 11 levels at 2^31 coefficients per row

// ---- the host's view of a code: shape, checked before anything reaches the device ---------------------------------------------------

struct BrakedownLayout {
  size_t msg_len = 0, m_ext = 0, n_levels = 0, nnz = 0;
  std::vector<size_t> a_n, a_m, b_n, b_m, start, end;      // BrakedownPCParams::new (brakedown.rs:163-181)
  std::vector<size_t> ptr_off, nnz_off;                    // matrix k (A matrices, then B matrices): where its ind_ptr / its entries start in the flat arrays
  size_t rss = 0, rs_in = 0, rsoe = 0;                     // base code: input cw[rss .. rss + rs_in), output cw[rss .. rsoe) (mod.rs:73-76)
};

// The checks of pc_hip_brakedown_code_create, as one plain host function: 0 = a code the kernels may run, otherwise the number of the
// first rule that failed (an out-of-range index never reaches a kernel).
//   dims: (n, m, d) per matrix, the n_levels A matrices first, then the n_levels B matrices; ind_ptr: m + 1 numbers per matrix, each
//   matrix counting its own entries from 0; col_ind: nnz_total row indices, the matrices' entries back to back.
inline int brakedown_validate(size_t msg_len, size_t codeword_len, size_t n_levels, const size_t* dims, const size_t* ind_ptr,
                              const uint32_t* col_ind, size_t nnz_total, BrakedownLayout* out) {
  static constexpr size_t LIM = (size_t)1 << 31;
  BrakedownLayout L;
  if (!msg_len || msg_len >= LIM || codeword_len >= LIM || codeword_len < msg_len) return 1;
  if (n_levels > SPRS_MAX_LEVELS) return 2;
  L.msg_len = msg_len; L.m_ext = codeword_len; L.n_levels = n_levels; L.nnz = nnz_total;
  if (!n_levels) {                                         // the base code alone (brakedown.rs:163-164: m_ext = ceil_mul(m, r), any length here)
    if (nnz_total) return 3;
    L.rss = 0; L.rs_in = msg_len; L.rsoe = codeword_len;
    if (out) *out = L;
    return 0;
  }
  if (!dims || !ind_ptr || (nnz_total && !col_ind)) return 3;
  for (size_t k = 0; k < 2 * n_levels; k++) {
    const size_t n = dims[3 * k], m = dims[3 * k + 1], d = dims[3 * k + 2];
    if (!n || !m || n >= LIM || m >= LIM || d > m) return 4;
    (k < n_levels ? L.a_n : L.b_n).push_back(n); (k < n_levels ? L.a_m : L.b_m).push_back(m);
  }
  if (L.a_n[0] != msg_len) return 5;
  for (size_t i = 0; i + 1 < n_levels; i++) if (L.a_n[i + 1] != L.a_m[i]) return 5;      // the A chain: level i + 1 reads what level i wrote
  size_t len = L.b_n[n_levels - 1];                                                       // codeword_len (brakedown.rs:292-299)
  for (size_t i = 0; i < n_levels; i++) { len += L.a_n[i] + L.b_m[i]; if (len >= LIM) return 6; }
  if (len != codeword_len) return 6;
  size_t s = 0, e = codeword_len;
  for (size_t i = 0; i < n_levels; i++) {
    s += L.a_n[i];
    if (L.b_m[i] > e) return 7;
    e -= L.b_m[i];
    if (e < s || L.b_n[i] != e - s) return 7;                                            // level i reads cw[start[i] .. end[i])
    L.start.push_back(s); L.end.push_back(e);
  }
  L.rss = L.start[n_levels - 1]; L.rs_in = L.a_m[n_levels - 1]; L.rsoe = L.end[n_levels - 1];
  if (L.rss + L.rs_in > codeword_len) return 7;
  size_t po = 0, no = 0;
  for (size_t k = 0; k < 2 * n_levels; k++) {
    const size_t n = dims[3 * k], m = dims[3 * k + 1], d = dims[3 * k + 2];
    const size_t* ip = ind_ptr + po;
    if (ip[0] != 0) return 8;
    for (size_t j = 0; j < m; j++) if (ip[j + 1] < ip[j] || ip[j + 1] - ip[j] > n) return 8;      // monotone; a column holds at most every row
    const size_t nnz = ip[m];
    if (nnz > n * d || nnz > nnz_total - no) return 9;
    for (size_t t = 0; t < nnz; t++) if (col_ind[no + t] >= n) return 10;
    L.ptr_off.push_back(po); L.nnz_off.push_back(no);
    po += m + 1; no += nnz;
  }
  if (no != nnz_total || no >= ((size_t)1 << 32)) return 9;
  if (out) *out = L;
  return 0;
}

// ---- the device's view ---------------------------------------------------------------------------------------------------------------

// one resident matrix inside an encode: output column j = sum over k in [ptr[j], ptr[j + 1]) of cw[in_pos + idx[k]] * val[k]
struct SprsDev {
  const uint32_t* ptr;      // m + 1 offsets into idx / val
  const uint32_t* idx;
  const uint32_t* val;      // Montgomery, 8 words per entry
  uint32_t m;               // output columns
  uint32_t clip;            // entries with idx >= clip read a place that is still zero in the reference (B products), = n for the A chain
  uint32_t in_pos, out_pos; // positions in the working buffer
};

// the matrices of a code as the kernels take them, and its base-code points 1, 2, 3, ... (Montgomery) -- all in one device allocation
struct BrakedownDev {
  uint32_t msg_len = 0, m_ext = 0, n_levels = 0;
  SprsDev a[SPRS_MAX_LEVELS], b[SPRS_MAX_LEVELS];
  uint32_t rss = 0, rs_in = 0, rsoe = 0;
  const uint32_t* points = nullptr;      // rsoe - rss of them
  uint32_t b_cols = 0;                   // output columns of all B products
  // positions of the working buffer: the codeword, then the input of the base code (its output overwrites the place the last A
  // product would have been appended to, so that product is written behind the codeword instead)
  uint32_t work_len() const { return m_ext + rs_in; }
};

// bytes of the device image of a code and the offsets of its parts (ptr arrays, idx, val, points), 32-byte aligned
struct BrakedownImage { size_t ptr_off = 0, idx_off = 0, val_off = 0, pts_off = 0, bytes = 0; };
inline BrakedownImage brakedown_image(const BrakedownLayout& L) {
  auto up = [](size_t b) { return (b + 31) & ~(size_t)31; };
  size_t ptrs = 0;
  for (size_t i = 0; i < L.n_levels; i++) ptrs += L.a_m[i] + 1 + L.b_m[i] + 1;
  BrakedownImage im;
  im.ptr_off = 0; im.idx_off = up(ptrs * 4); im.val_off = im.idx_off + up(L.nnz * 4); im.pts_off = im.val_off + L.nnz * 32;
  im.bytes = im.pts_off + (L.rsoe - L.rss) * 32;
  return im;
}
// fill the host copy of the image (ind_ptr narrowed to 32 bits and made absolute; col_ind, val and the points copied) and the descriptor
// whose pointers are `base` + offsets.  points_mont: rsoe - rss field elements.
inline void brakedown_fill(const BrakedownLayout& L, const size_t* ind_ptr, const uint32_t* col_ind, const void* val, const uint32_t* points_mont,
                           uint8_t* host, const uint8_t* base, BrakedownDev* D) {
  const BrakedownImage im = brakedown_image(L);
  uint32_t* hp = (uint32_t*)(host + im.ptr_off);
  if (L.nnz) { memcpy(host + im.idx_off, col_ind, L.nnz * 4); memcpy(host + im.val_off, val, L.nnz * 32); }
  memcpy(host + im.pts_off, points_mont, (L.rsoe - L.rss) * 32);
  BrakedownDev d;
  d.msg_len = (uint32_t)L.msg_len; d.m_ext = (uint32_t)L.m_ext; d.n_levels = (uint32_t)L.n_levels;
  d.rss = (uint32_t)L.rss; d.rs_in = (uint32_t)L.rs_in; d.rsoe = (uint32_t)L.rsoe;
  d.points = (const uint32_t*)(base + im.pts_off);
  size_t pw = 0;
  for (size_t k = 0; k < 2 * L.n_levels; k++) {
    const bool is_a = k < L.n_levels; const size_t i = is_a ? k : k - L.n_levels;
    const size_t m = is_a ? L.a_m[i] : L.b_m[i];
    for (size_t j = 0; j <= m; j++) hp[pw + j] = (uint32_t)(L.nnz_off[k] + ind_ptr[L.ptr_off[k] + j]);
    SprsDev& s = is_a ? d.a[i] : d.b[i];
    s.ptr = (const uint32_t*)(base + im.ptr_off) + pw; s.idx = (const uint32_t*)(base + im.idx_off); s.val = (const uint32_t*)(base + im.val_off);
    s.m = (uint32_t)m;
    if (is_a) {
      s.clip = (uint32_t)L.a_n[i]; s.in_pos = (uint32_t)(L.start[i] - L.a_n[i]);
      s.out_pos = i + 1 == L.n_levels ? (uint32_t)L.m_ext : (uint32_t)L.start[i];
    } else {
      // level i reads cw[start[i] .. end[i]); what lies at or above end[last] is written by the levels after it and is still zero
      // when the reference's loop (mod.rs:79-82, level 0 first) reaches level i
      s.clip = (uint32_t)(L.rsoe - L.start[i]); s.in_pos = (uint32_t)L.start[i]; s.out_pos = (uint32_t)L.end[i];
      d.b_cols += (uint32_t)m;
    }
    pw += m + 1;
  }
  *D = d;
}

// ---- kernel bodies (one lane = one call of operator()) -------------------------------------------------------------------------------

// row-major src[r * stride + pos] -> T[(pos0 + pos) * rows + r]; lane g: row g % rows, positions 4 (g / rows) .. + 4
template <class FrP>
struct SprsTransposeInBody {
  const uint32_t* src; uint32_t stride, len, rows, pos0; uint32_t* T;
  PC_HD void operator()(uint32_t g) const {
    const uint32_t q = g / rows, r = g - q * rows;
    for (uint32_t k = 0; k < 4; k++) {
      const uint32_t pos = 4 * q + k;
      if (pos >= len) return;
      Fd<FrP>::load(src + ((size_t)r * stride + pos) * FrP::N).store(T + ((size_t)(pos0 + pos) * rows + r) * FrP::N);
    }
  }
};
// T[pos * rows + r] -> row-major dst[r * len + pos]
template <class FrP>
struct SprsTransposeOutBody {
  const uint32_t* T; uint32_t len, rows; uint32_t* dst;
  PC_HD void operator()(uint32_t g) const {
    const uint32_t q = g / rows, r = g - q * rows;
    for (uint32_t k = 0; k < 4; k++) {
      const uint32_t pos = 4 * q + k;
      if (pos >= len) return;
      Fd<FrP>::load(T + ((size_t)pos * rows + r) * FrP::N).store(dst + ((size_t)r * len + pos) * FrP::N);
    }
  }
};

// the batched sparse product of n_mats matrices in one launch: lane g owns row g % rows of output column g / rows, the columns of the
// matrices counted through
template <class FrP>
struct SprsMulBody {
  typedef Fd<FrP> F;
  uint32_t* T; uint32_t rows, n_mats; SprsDev mats[SPRS_MAX_LEVELS];
  PC_HD F elem(const SprsDev& M, uint32_t k, uint32_t r) const {
    const uint32_t i = M.idx[k];
    return i < M.clip ? F::load(T + ((size_t)(M.in_pos + i) * rows + r) * FrP::N) : F::zero();
  }
  PC_HD void operator()(uint32_t g) const {
    uint32_t j = g / rows; const uint32_t r = g - j * rows;
    uint32_t w = 0;
    while (w + 1 < n_mats && j >= mats[w].m) { j -= mats[w].m; w++; }
    const SprsDev& M = mats[w];
    uint32_t k = M.ptr[j]; const uint32_t ke = M.ptr[j + 1];
    F acc = F::zero();
    for (; k + 1 < ke; k += 2)
      acc = acc.add(elem(M, k, r).mul_add_mul(F::load(M.val + (size_t)k * FrP::N), elem(M, k + 1, r), F::load(M.val + (size_t)(k + 1) * FrP::N)));
    if (k < ke) acc = acc.add(elem(M, k, r).mul(F::load(M.val + (size_t)k * FrP::N)));
    acc.store(T + ((size_t)(M.out_pos + j) * rows + r) * FrP::N);
  }
};

// naive_reed_solomon (mod.rs:111-122): Horner over the rs_in inputs, highest first, at the point g / rows + 1 for row g % rows
template <class FrP>
struct SprsBaseCodeBody {
  typedef Fd<FrP> F;
  uint32_t* T; uint32_t rows, in_pos, in_len, out_pos; const uint32_t* points;
  PC_HD void operator()(uint32_t g) const {
    const uint32_t p = g / rows, r = g - p * rows;
    const F x = F::load(points + (size_t)p * FrP::N);
    F acc = F::zero();
    for (uint32_t j = in_len; j-- > 0;) acc = acc.mul(x).add(F::load(T + ((size_t)(in_pos + j) * rows + r) * FrP::N));
    acc.store(T + ((size_t)(out_pos + p) * rows + r) * FrP::N);
  }
};

// ---- one encode: rows messages (row-major, msg_len each) -> rows codewords (row-major, m_ext each) ------------------------------------
// T: working buffer of work_len() * rows elements.  be.mark() is called after the base code and after the B products (phase brackets).
template <class FrP, class Backend>
void brakedown_encode(Backend& be, const BrakedownDev& D, const uint32_t* msgs, uint32_t rows, uint32_t* T, uint32_t* out) {
  auto lanes = [&](uint32_t positions) { return (size_t)positions * rows; };
  // the message: the head of the codeword -- or, without levels, the input of the base code
  SprsTransposeInBody<FrP> tin{msgs, D.msg_len, D.msg_len, rows, D.n_levels ? 0u : D.m_ext, T};
  be.launch(tin, lanes((D.msg_len + 3) / 4));
  for (uint32_t i = 0; i < D.n_levels; i++) {              // the A chain (mod.rs:65-68): each level reads the one before
    SprsMulBody<FrP> mul{T, rows, 1u, {}}; mul.mats[0] = D.a[i];
    be.launch(mul, lanes(D.a[i].m));
  }
  SprsBaseCodeBody<FrP> rs{T, rows, D.m_ext, D.rs_in, D.rss, D.points};
  be.launch(rs, lanes(D.rsoe - D.rss));
  be.mark();
  if (D.n_levels) {                                        // every B product (mod.rs:79-82), clipped: see the head of this file
    SprsMulBody<FrP> mul{T, rows, D.n_levels, {}};
    for (uint32_t i = 0; i < D.n_levels; i++) mul.mats[i] = D.b[i];
    be.launch(mul, lanes(D.b_cols));
  }
  be.mark();
  SprsTransposeOutBody<FrP> tout{T, D.m_ext, rows, out};
  be.launch(tout, lanes((D.m_ext + 3) / 4));
}

// the points 1, 2, .., count of the base code in Montgomery form (host)
template <class FrP>
void brakedown_points(uint32_t* out, size_t count) {
  Fd<FrP> x = Fd<FrP>::one();
  for (size_t i = 0; i < count; i++) { x.store(out + i * FrP::N); x = x.add(Fd<FrP>::one()); }
}

}  // namespace pc
