// Internal interfaces between the translation units of libpc_hip.so.
//
// The library is built from several .hip files compiled in parallel (poly_commit_amd/build.py):
//   abi_<subject>.hip  the extern "C" entry points (include/pc_hip.h), one unit per subject: ctx (context, errors, memory, timing),
//                      srs (keys and their tables), msm, poly (polynomials, NTT, hashing, Ligero), ipa, lincode (the Brakedown code object),
//                      skzg (streaming_kzg: folding tree, multi-point openings), pst13 (MarlinPST13: layout, commit, open); staging,
//                      error translation
//   key.hpp            host only: the key objects -- pc_key_base and what the keys of every group share over it (fill, read-back,
//                      registry, locked free, key_make: one new key or nothing), pc_srs with its pipelines and the derived keys of an
//                      opening, pc_g2_srs and pc_te_srs with their BlockingLane (residency, trim) -- their whole lifetime
//   abi.hpp            host only: the staging helpers more than one abi unit uses
//   abi_fr.hpp         host only: the entry points over a scalar field's vector kernels (FrVecOps below), written once for the fields
//                      of pc_curve (abi_ipa.hip, abi_poly.hip) and for ed_on_bls12_381's (abi_te_ipa.hip)
//   curve_<name>.hip   everything templated on one curve: MSM pipeline, window table, key fold, fixed-base mul, pair sums
//   abi_g2.hip         beside its entry points, everything templated on G2 (BLS12-381 only); it instantiates no G1 kernel
//   abi_te.hip         the same for the twisted Edwards group ed_on_bls12_381 (te.hpp): typed keys, MSM, many-MSM pass, key fold
//   blocking_lane.hpp  the blocking MSM lane of those two groups (BlockingRunner below over MsmPlan<G, HipBackend>): one copy, included
//                      by abi_g2.hip and abi_te.hip alone, each instantiating it for its own group
//   abi_te.hpp         what the three twisted Edwards units share: the group's names and sizes, the id check, the normalisation tail
//   abi_te_setup.hip   sample_generators and the prefix of a twisted Edwards key (te_setup.hpp)
//   abi_setup.hip      sample_generators and the prefix of a key over the short Weierstrass curves (sw_setup.hpp): it instantiates the
//                      sampling kernels of all four curves itself
//   abi_te_ipa.hip     the FrVecOps table of ed_on_bls12_381's scalar field (no NTT, no FieldOps entry) and the opening as one call
//   fixed_base.hpp     the group-generic launch sequences (fixed-base batch multiplication, pair sums): one copy, instantiated for
//                      G1 by the curve units and for G2 by abi_g2.hip
//   host_tail.hpp      host only: 64-bit-limb points of either group -- the MSM's Horner tail, affine -> XYZZ, one scalar
//                      multiplication, a sum of points, the fixed base's window table
//   field_<name>.hip   everything templated on one scalar field: NTT, division scan, IPA vector kernels,
//                      column digests, the Brakedown encoder (sprs.hpp), the folding tree and multi-point division (skzg.hpp),
//                      MarlinPST13's monomial evaluations, scatter and division along a variable (pst13.hpp)
// The abi units reach the templates through the two tables of plain function pointers below, one
// instance per curve / field.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdexcept>
#include "../../include/pc_hip.h"
#include "curves.hpp"
#include "hip_backend.hpp"
#include "msm.hpp"
#include "sprs.hpp"

namespace pc {

struct MsmRunner {
  virtual ~MsmRunner() {}
  virtual void enqueue(const uint32_t* bases, uint32_t base_off, const void* scalars, pc_mem where, size_t n, bool from_mont) = 0;
  // many-MSM runners only: `count` scalar vectors of m elements each in separate device buffers (a batch of polynomials)
  virtual void enqueue_vectors(const uint32_t* bases, uint32_t base_off, const uint64_t* ptrs_host, size_t count, size_t m, bool from_mont) = 0;
  // ONE MSM of n_total pairs in parts (MsmPlan::begin_parts): part k covers scalars [first, first + n) of the call -- host memory: copied on
  // the pipeline's auxiliary queue; device memory: readable now -- against bases base_off + first ..; `last` closes the call
  virtual void begin_parts(size_t n_total) = 0;
  virtual void add_part(const uint32_t* bases, uint32_t base_off, size_t first, const void* scalars_part, pc_mem where, size_t n, bool from_mont, bool last) = 0;
  virtual void finish(uint32_t* out_host) = 0;
  // geometry of the last enqueue: {window bits c, signed digits per scalar, buckets, 1 if the window table was used}
  virtual void shape(uint32_t out[4]) const = 0;
  virtual void trim() = 0;          // give back what can be rebuilt on demand (idle pipeline only)
};

// One blocking MSM pipeline of G2 or of the twisted Edwards group (blocking_lane.hpp: MsmPlan<G, HipBackend>; abi_g2.hip and abi_te.hip
// each make their own group's)
struct BlockingRunner {
  virtual ~BlockingRunner() {}
  // out_host: the affine sum(s) -- G2: 4 Fq (all zero = infinity); twisted Edwards: x || y, 2 Fq (the identity is (0, 1)), n >= 1
  virtual void run(const uint32_t* bases, uint32_t base_off, const void* scalars, pc_mem where, size_t n, bool from_mont, uint32_t* out_host) = 0;
  // geometry of the last run, as MsmRunner::shape reports it
  virtual void shape(uint32_t out[4]) const = 0;
};

struct NttRunner {
  virtual ~NttRunner() {}
  virtual void run(const uint32_t* in, size_t rows, size_t in_cols, uint32_t* out) = 0;
};

// CurveOps::fixed_base / fixed_base_run<G>: results normalised around one inversion per K.  16 for pc_hip_fixed_base_batch_mul (the
// SRS generation of KZG10::setup), 8 for the two groups of MultilinearPC (pc_hip_ml_setup, pc_hip_g2_fixed_base_batch_mul): with 16 the
// G1 level of the setup measured 0.3 ms slower at 2^20 (profiles/EXPERIMENTS.md 000000).
constexpr uint32_t FIXED_BASE_K_KZG = 16, FIXED_BASE_K_ML = 8;

struct CurveOps {
  int aw;                 // 32-bit words per affine point
  uint32_t scalar_bits;
  MsmRunner* (*make_runner)(HipBackend& be, size_t n_max, const MsmConfig& cfg, uint32_t subs);
  void (*window_table)(HipBackend& be, const uint32_t* bases, uint32_t n, uint32_t c, uint32_t Wd, uint32_t* table, uint32_t stride);
  // out[i] = affine(in[i] + u * in[half + i]); table: the key's one-level fold table of width-w NAF digits (or null: GLV ladder).  out == in: in place.
  void (*ec_fold_to)(HipBackend& be, const uint32_t* in, uint32_t* out, size_t half, const uint32_t* u_mont, const uint32_t* table, uint32_t w);
  // out[i] = affine(key_lo[i] + sum_t u_t * P_t[i]) from the fold table (term t = table points [t count, (t + 1) count)); false: does not fit
  bool (*ec_fold_table)(HipBackend& be, const uint32_t* key_lo, uint32_t* out, size_t count, size_t row_pts, uint32_t terms,
                        const uint32_t* const* u_monts, uint32_t w, const uint32_t* table);
  // fold table of `count` key points for width-w NAF digits: 2^(w-2) * fold_rows rows of `count` points
  void (*fold_table_build)(HipBackend& be, const uint32_t* pts, size_t count, uint32_t w, uint32_t* table);
  uint32_t fold_rows;
  // out[i] = scalars[i] * g for one affine point g (host) and n Montgomery scalars on the device; one inversion per K results (fixed_base.hpp)
  void (*fixed_base)(HipBackend& be, const uint32_t* g, const uint32_t* scalars, size_t n, uint32_t* out, uint32_t K);
  // out[b] = in[2b] + in[2b + 1], b < count, affine points on the device; `in` and `out` must not overlap
  void (*pair_sums)(HipBackend& be, const uint32_t* in, size_t count, uint32_t* out);
  // ark-serialize bytes of n points (device) -> n resident affine points; returns the number of invalid points
  uint32_t (*srs_decode)(HipBackend& be, const uint8_t* bytes_dev, size_t n, int compressed, uint32_t* out);
  // n resident affine points -> their ark-serialize bytes (device buffers)
  void (*srs_encode)(HipBackend& be, const uint32_t* pts_dev, size_t n, int compressed, uint8_t* out_dev);
  // host-side helpers (a handful of points, as the reference does on the host)
  void (*points_sum)(const uint32_t* pts, size_t count, uint32_t* out);
  void (*point_mul)(const uint32_t* pt, const uint32_t* k_mont, uint32_t* out);
  void (*fr_mul)(const uint32_t* a_mont, const uint32_t* b_mont, uint32_t* out_mont);      // one scalar-field product on the host
  void (*fr_inv)(const uint32_t* a_mont, uint32_t* out_mont);                             // a^-1 (0 -> 0), host
  void (*fr_one)(uint32_t* out_mont);
};

// streaming_kzg: coefficients of one tile (skzg.hpp: what one workgroup folds or divides in LDS), one polynomial of a division
// (q: max(len - k, 0) coefficients; longer than a tile: the element in front of q is written too), the division's scratch
constexpr uint32_t SKZG_TILE = 1024;
struct SkzgDivLevel { const uint32_t* src; uint32_t len; uint32_t* q; };
inline size_t skzg_div_scratch_bytes(size_t max_len, size_t count, uint32_t k) {
  return (2 * (max_len > SKZG_TILE ? max_len : 0) + count * k + k) * 32 + count * 24 + 64;
}

// The vector kernels of the IPA rounds and of Hyrax's opening: all that exists over a scalar field without an NTT (abi_te_ipa.hip
// makes this table alone for ed_on_bls12_381's field, which has no pc_curve id; abi_fr.hpp holds the entry points over it)
constexpr size_t FR_BYTES = 32;      // one element of any of the scalar fields here: 8 words (FieldOpsImpl asserts it)
struct FrVecOps {
  void (*fr_dot)(HipBackend& be, const uint32_t* a, const uint32_t* b, size_t n, uint32_t* out_host);
  void (*ipa_fold_dots)(HipBackend& be, uint32_t* c, uint32_t* z, size_t m, const uint32_t* u_host, const uint32_t* u_inv_host, uint32_t* out_host);
  void (*fr_powers)(HipBackend& be, const uint32_t* z, size_t n, uint32_t* out);
  void (*ipa_key_scalars)(HipBackend& be, const uint32_t* c, size_t m, uint32_t* s, size_t n0, const uint32_t* fold_u, size_t fold_m,
                          uint32_t* out_l, uint32_t* out_r);
  void (*fr_lincomb)(HipBackend& be, const void* addr, const void* lens, const void* xi, size_t k, void* out, size_t n_out);
};

struct FieldOps : FrVecOps {
  NttRunner* (*make_ntt)(HipBackend& be, unsigned log_n);
  void (*poly_eval)(HipBackend& be, const uint32_t* x, size_t n, const uint32_t* z_host, uint32_t* out_host, uint32_t fan);
  void (*div_scan)(HipBackend& be, const uint32_t* x, size_t n, const uint32_t* z_host, const uint32_t* carry_in_host, uint32_t* out,
                   uint32_t fan);
  void (*witness)(HipBackend& be, const uint32_t* p, size_t n, const uint32_t* z_host, uint32_t* q, uint32_t fan);
  void (*fr_fold)(HipBackend& be, uint32_t* lo, const uint32_t* hi, size_t n, const uint32_t* s);
  void (*column_hash)(HipBackend& be, int hash, const uint32_t* ext, uint32_t rows, uint32_t n_cols, uint32_t* out);
  // one slab of rows absorbed into the per-column chaining states (hash.hpp, ColumnHashPartBody); columns [col0, col0 + cols)
  void (*column_hash_part)(HipBackend& be, int hash, const uint32_t* ext, uint32_t rows, uint32_t n_cols, uint32_t rows_total, uint32_t col0,
                           uint32_t cols, int first, int last, uint32_t* state, uint32_t* out);
  // one Brakedown encode of `rows` messages (sprs.hpp): row-major in and out, T = the transposed working buffer; two phase marks
  void (*brakedown_encode)(HipBackend& be, const BrakedownDev& code, const uint32_t* msgs, uint32_t rows, uint32_t* T, uint32_t* out);
  void (*brakedown_points)(uint32_t* out_host, size_t count);      // the base code's points 1, 2, .. in Montgomery form (host)
  // streaming_kzg (skzg.hpp): every level of the folding tree into out at the element offsets offs_host; `count` polynomials divided by
  // one vanishing polynomial, remainders on the host (highest degree first).  Both return their number of kernel launches.
  uint32_t (*fold_tree)(HipBackend& be, const uint32_t* f, size_t n, const uint32_t* rho_host, uint32_t depth, uint32_t* out, const uint64_t* offs_host);
  uint32_t (*div_multi)(HipBackend& be, const SkzgDivLevel* lv, size_t count, const uint32_t* z_host, uint32_t k, uint32_t* rem_host, void* scratch,
                        uint32_t fan);
  // MarlinPST13 (pst13.hpp), on the layout (n, d) with its table T of (n + 1)(d + 1) words on the device.  None drains the stream.
  // out[rank] = prod_j pw[j][e_j] for every rank; pw: n x (d + 1) powers on the device
  void (*pst13_monomials)(HipBackend& be, const uint32_t* table, uint32_t n, uint32_t d, size_t len, const uint32_t* pw, uint32_t* out);
  // the second pass of the scatter: every term that owns its slot writes its coefficient, the others raise PST13_FLAG_REPEATED
  void (*pst13_write)(HipBackend& be, const uint32_t* table, uint32_t n, uint32_t d, const uint8_t* exps, const uint32_t* coeffs, size_t terms,
                      const uint32_t* owner, uint32_t* flags, uint32_t* out);
  // the n passes of the division (n >= 2): see pst13_divide; returns the device buffer whose slot 0 holds p(z)
  const uint32_t* (*pst13_divide)(HipBackend& be, const uint32_t* table, const uint32_t* T_host, uint32_t n, uint32_t d, const uint32_t* p,
                                  const uint32_t* z_host, uint32_t* quot, const uint64_t* offs, uint32_t* ping, uint32_t* pong);
};

// (accessor functions rather than global tables: a namespace-scope constant would also be emitted into the
// device image, where the host function addresses do not exist)
const CurveOps& curve_ops_bls12_381(); const CurveOps& curve_ops_bn254(); const CurveOps& curve_ops_pallas(); const CurveOps& curve_ops_bls12_377();
const FieldOps& field_ops_bls12_381(); const FieldOps& field_ops_bn254(); const FieldOps& field_ops_pallas(); const FieldOps& field_ops_bls12_377();
const FrVecOps& fr_vec_ops_ed_on_bls12_381();      // abi_te_ipa.hip

// (the entry points have refused every id outside [0, PC_CURVE_LAST], curves.hpp, before they come here)
inline const CurveOps& curve_ops(pc_curve c) {
  switch (c) {
    case PC_CURVE_BLS12_381: return curve_ops_bls12_381();
    case PC_CURVE_BN254: return curve_ops_bn254();
    case PC_CURVE_PALLAS: return curve_ops_pallas();
    case PC_CURVE_BLS12_377: return curve_ops_bls12_377();
  }
  throw std::invalid_argument("unknown curve id");
}
inline const FieldOps& field_ops(pc_curve c) {
  switch (c) {
    case PC_CURVE_BLS12_381: return field_ops_bls12_381();
    case PC_CURVE_BN254: return field_ops_bn254();
    case PC_CURVE_PALLAS: return field_ops_pallas();
    case PC_CURVE_BLS12_377: return field_ops_bls12_377();
  }
  throw std::invalid_argument("unknown curve id");
}

// hash-only kernels (hash_tu.hip)
void gather_columns(HipBackend& be, const uint32_t* mat, size_t rows, size_t n_cols, const uint32_t* idx_dev, size_t t, uint32_t* out);
void merkle_level(HipBackend& be, int hash, const uint32_t* child, uint32_t* parent, uint32_t n_leaves, uint32_t bottom,
                  uint32_t len_prefix, size_t cnt);

}  // namespace pc
