// BLS12-381 Fq in radix 2^30: 13 limbs of 30 bits in 32-bit words, Montgomery form for R' = 2^390.
//
// Why: in fp32.hpp's radix 2^32 every partial product costs a v_mad_u64_u32 AND a v_addc_co_u32 (the multiply-add has no carry-in, so
// the 96-bit column needs its top word carried by hand).  With 30-bit limbs a whole column -- up to 13 products a_i b_j and 13
// reduction terms m_i p_j, each below 2^60 -- fits the 64-bit accumulator of the multiply-add itself: 2 * 13^2 = 338 multiplies per
// product and no carry instruction, against 288 + 288.  The spare 9 bits of R' (R'/p = 630.05) also make every value of the mixed
// addition lazily reduced for free: no conditional subtraction anywhere, differences are made non-negative by adding a multiple of p.
//
// Only the running sum of the bucket accumulation lives in this form (ec.hpp XyzzR30, msm.hpp AccumulateBody).  Memory keeps the
// 12-word R = 2^384 layout:
//   load   a canonical 12-word residue w = x 2^384 mod p, shifted left by 6 bits and re-cut into 13 limbs, IS x 2^390 = x R' up to
//          multiples of p (64 w, below 64p): from32(), two bit operations per limb, no multiplication
//   store  the exact division by 64 modulo p (add k p, k = -v p^-1 mod 64, shift right by 6) takes x R' back to x 2^384, below 2p:
//          to32(), re-packed into 12 words -- the lazily reduced form the consumers of the accumulation take already (fp32.hpp
//          LAZY_STORE_OK); no multiplication either
//
// Operand classes.  A value "of class V" is an integer in [0, V p] whose limbs 0..11 are below 2^30; limb 12 holds the rest
// (at most V (p >> 360), lmax()).  Every function states the classes it takes and returns; the multiplier templates carry them as
// parameters because the column bounds depend on them (below).  With p/R' < 1/630 a Montgomery product (a b + m p)/R', m < R', of
// classes VA, VB is below (VA VB / 630 + 1) p: class mul_out(VA VB) = VA VB / 630 + 2 (integer division).
//
// Column bounds.  13 + 13 terms below 2^60 do NOT all fit 64 bits: with worst-case limbs the middle columns of a product reach 65
// bits, those of the fused pair (26 + 13 terms) 66.  plan() walks the columns at compile time with the limb bounds of the operand
// classes and the actual limbs of p, and where the accumulator could overflow before the next group of terms it moves the
// accumulator's high word aside (added back, shifted, when the column closes).  The result is checked by static_assert (Plan::ok);
// no column is listed by hand.
//
// Host and device compute the same integers: Montgomery's m is determined by the sum alone, so the host's row-wise form is the
// device's column-wise one bit for bit (tests/emu steps the real ranges; tests/hip runs every instantiation XyzzR30::add_affine makes
// on the device, on the boundary values of its operand classes: tests/test_device_primitives_gpu.py).
// (tests/test_emu_cpu.py rebuilds tests/emu/libemu.so when one of the headers it lists is newer; this header is not in that list:
// remove the library after editing it.)
#pragma once
#include "fp32.hpp"

// product switch (poly_commit_amd/build.py, PC_HIP_CXXFLAGS): 0 keeps the running sum of the BLS12-381 accumulation in radix 2^32
#ifndef PC_ACC_R30
#define PC_ACC_R30 1
#endif

namespace pc {

// compile-time helpers of Fq30 (a separate, complete type: Fq30 initialises its constants with them)
struct Fq30Const {
  typedef pc_bls12_381_fq P;
  typedef unsigned __int128 u128;
  static constexpr int N = 13;
  static constexpr uint32_t MASK = (1u << 30) - 1;
  // ---- constants, all derived from field_constants.h at compile time ------------------------------------------------------
  struct L13 { uint32_t v[N]; };
  struct W12 { uint32_t w[12]; };
  // 12 words (shifted left by S bits) re-cut into 13 limbs of 30 bits; the value must stay below 2^390
  static constexpr L13 recut_c(const uint32_t* w, int S) {
    L13 r{};
    for (int i = 0; i < N; i++) {
      uint32_t v = 0;
      for (int b = 0; b < 30; b++) {
        const int src = 30 * i + b - S;
        if (src >= 0 && src < 384) v |= ((w[src >> 5] >> (src & 31)) & 1u) << b;
      }
      r.v[i] = v;
    }
    return r;
  }
  // limbs of V p
  static constexpr L13 kp(int V) {
    uint32_t w[13] = {};
    uint64_t c = 0;
    for (int i = 0; i < 12; i++) { c += (uint64_t)P::MOD[i] * (uint32_t)V; w[i] = (uint32_t)c; c >>= 32; }
    w[12] = (uint32_t)c;
    L13 r{};
    for (int i = 0; i < N; i++) {
      uint32_t v = 0;
      for (int b = 0; b < 30; b++) { const int src = 30 * i + b; if (src < 416) v |= ((w[src >> 5] >> (src & 31)) & 1u) << b; }
      r.v[i] = v;
    }
    return r;
  }
  // 2^(384 + S) mod p as 12 words, from ONE = 2^384 mod p by S modular doublings
  static constexpr W12 pow2_c(int S) {
    W12 x{};
    for (int i = 0; i < 12; i++) x.w[i] = P::ONE[i];
    for (int s = 0; s < S; s++) {
      uint32_t c = 0;
      for (int i = 0; i < 12; i++) { const uint32_t t = x.w[i]; x.w[i] = (t << 1) | c; c = t >> 31; }      // < 2p < 2^384
      uint32_t d[12] = {}; uint64_t br = 0;
      for (int i = 0; i < 12; i++) { const uint64_t t = (uint64_t)x.w[i] - P::MOD[i] - br; d[i] = (uint32_t)t; br = t >> 63; }
      if (br == 0) for (int i = 0; i < 12; i++) x.w[i] = d[i];
    }
    return x;
  }
  // ---- column plan ----------------------------------------------------------------------------------------------------------
  enum { MUL = 0, SQR = 1, DUAL = 2 };
  // largest limb i of a value of class V: p < (MOD[11] + 1) 2^352, limb 12 = value >> 360
  static constexpr uint64_t lmax(int V, int i) { return i < N - 1 ? (uint64_t)MASK : ((uint64_t)V * ((uint64_t)P::MOD[11] + 1)) >> 8; }
  // split[k][g]: the high word of the accumulator is moved aside before group g of column k (0: products a_i b_j, or the squaring's
  // terms; 1: products c_i d_j of the fused pair; 2: reduction terms m_i p_j, with the closing m_k p_0 of a low column)
  struct Plan { bool split[2 * N - 1][3]; bool ok; };
  static constexpr Plan plan(int kind, int VA, int VB, int VC, int VD) {
    Plan pl{};
    pl.ok = lmax(VA, N - 1) <= MASK && lmax(VB, N - 1) <= MASK && lmax(VC, N - 1) <= MASK && lmax(VD, N - 1) <= MASK;
    const u128 U64MAX = ~(uint64_t)0;
    u128 carry = 0;
    for (int k = 0; k < 2 * N - 1; k++) {
      const int i0 = k > N - 1 ? k - (N - 1) : 0, i1 = k < N - 1 ? k : N - 1;
      u128 g[3] = {0, 0, 0};
      for (int i = i0; i <= i1; i++) {
        const int j = k - i;
        if (kind == SQR) { if (i < j) g[0] += (u128)lmax(VA, i) * (2 * lmax(VA, j)); else if (i == j) g[0] += (u128)lmax(VA, i) * lmax(VA, i); }
        else { g[0] += (u128)lmax(VA, i) * lmax(VB, j); if (kind == DUAL) g[1] += (u128)lmax(VC, i) * lmax(VD, j); }
        g[2] += (u128)MASK * kp(1).v[j];
      }
      u128 acc = carry, aside = 0;
      for (int gi = 0; gi < 3; gi++) {
        if (g[gi] == 0) continue;
        if (acc + g[gi] > U64MAX) {
          pl.split[k][gi] = true;
          aside += acc >> 32; acc = 0xffffffffu;
          if (acc + g[gi] > U64MAX) pl.ok = false;
        }
        acc += g[gi];
      }
      carry = (acc >> 30) + (aside << 2);
      if (carry > U64MAX || aside > U64MAX) pl.ok = false;
    }
    if (carry > 0xffffffffu) pl.ok = false;      // the top limb of the result is one word
    return pl;
  }
};

struct Fq30 : Fq30Const {
  typedef Fd<P> F32;
  uint32_t l[N];

  // ---- constants, all derived from field_constants.h at compile time ------------------------------------------------------
  static constexpr L13 PL = kp(1);                                   // limbs of p
  static constexpr uint32_t INV30 = P::INV & MASK;                    // -p^-1 mod 2^30
  static constexpr uint32_t PINV30 = (0u - P::INV) & MASK;            // p^-1 mod 2^30
  static constexpr W12 ONE390 = pow2_c(6);
  static constexpr L13 ONE30 = recut_c(ONE390.w, 0);                  // 1 in this form: 2^390 mod p, class 1
  static_assert(((uint64_t)PL.v[0] * INV30 & MASK) == MASK, "INV30 = -p^-1 mod 2^30");
  // R'/p >= 630: p < (MOD[11] + 1) 2^352 and 630 (MOD[11] + 1) <= 2^38
  static_assert((uint64_t)630 * ((uint64_t)P::MOD[11] + 1) <= ((uint64_t)1 << 38), "p/R' < 1/630");
  static constexpr int mul_out(int prod) { return prod / 630 + 2; }   // class of (a b [+ c d] + m p)/R' for VA VB [+ VC VD] = prod

  static PC_HD Fq30 zero() { Fq30 r; PC_UNROLL for (int i = 0; i < N; i++) r.l[i] = 0; return r; }
  static PC_HD Fq30 of(const L13& c) { Fq30 r; PC_UNROLL for (int i = 0; i < N; i++) r.l[i] = c.v[i]; return r; }
  static PC_HD Fq30 one() { constexpr L13 c = ONE30; return of(c); }                                      // class 1
  // the integer 0 (limbs are normalised, so the representation of an integer is unique)
  PC_HD bool is_zero_exact() const { uint32_t a = 0; PC_UNROLL for (int i = 0; i < N; i++) a |= l[i]; return a == 0; }

  // ---- conversions ---------------------------------------------------------------------------------------------------------
  // 12 words w (R = 2^384 form, w <= V32 p) -> 64 w: the same residue in R' = 2^390 form, class 64 V32 (canonical or p itself: 64)
  static PC_HD Fq30 from32(const F32& w) {
    Fq30 r;
    r.l[0] = (w.l[0] << 6) & MASK;
    PC_UNROLL for (int i = 1; i < N; i++) {
      const int o = 30 * i - 6, j = o >> 5, s = o & 31;                                                    // limb i = bits [o, o + 30) of w
      const uint64_t two = (uint64_t)w.l[j] | (j + 1 < 12 ? (uint64_t)w.l[j + 1] << 32 : 0);
      r.l[i] = (uint32_t)(two >> s) & MASK;
    }
    return r;
  }
  // class 64 -> 12 words, R = 2^384 form, below 2p: the inverse of from32 is an exact division by 64 modulo p -- add k p with
  // k = -v p^-1 mod 64 (a six-bit Montgomery step: the low six bits become zero), shift right by 6 while re-packing into words.
  // (v + k p)/64 <= (64p + 63p)/64 < 2p.  13 small multiply-adds: this runs in the accumulation's boundary block, which a wave enters
  // whenever ONE of its lanes ends a bucket run (half of the iterations at 2^24) -- a full product per coordinate there cost what the
  // carry-free products had saved
  PC_HD F32 to32() const {
    constexpr L13 Pl = PL;
    const uint32_t k = (l[0] * INV30) & 63u;
    uint32_t t[N]; uint64_t c = 0;
    PC_UNROLL for (int i = 0; i < N - 1; i++) { c += (uint64_t)k * Pl.v[i] + l[i]; t[i] = (uint32_t)c & MASK; c >>= 30; }
    t[N - 1] = l[N - 1] + k * Pl.v[N - 1] + (uint32_t)c;                                                   // < 2^28
    F32 r;
    PC_UNROLL for (int j = 0; j < 12; j++) {
      const int o = 32 * j + 6, q = o / 30, s = o % 30;                                                    // s <= 28: two limbs cover the word
      const uint64_t two = (uint64_t)t[q] | ((uint64_t)t[q + 1] << 30);
      r.l[j] = (uint32_t)(two >> s);
    }
    return r;
  }
  // class 64 -> class 2, same residue: product with 1 (2^390 mod p)
  PC_HD Fq30 reduce() const { return mul<64, 1>(*this, one()); }

  // ---- additive operations: results kept non-negative by adding V p, limbs renormalised by a signed carry -----------------
  // a - b + V p.  Needs b <= V p.  Class: (class of a) + V.   Per limb a_i - b_i + K_i + c lies in [-2^30, 2^31): one int32
  template <int V>
  static PC_HD Fq30 sub(const Fq30& a, const Fq30& b) {
    constexpr L13 K = kp(V);
    Fq30 r; int32_t c = 0;
    PC_UNROLL for (int i = 0; i < N - 1; i++) {
      const int32_t t = (int32_t)(a.l[i] - b.l[i] + K.v[i]) + c;
      r.l[i] = (uint32_t)t & MASK; c = t >> 30;
    }
    r.l[N - 1] = a.l[N - 1] - b.l[N - 1] + K.v[N - 1] + (uint32_t)c;      // the value is non-negative, so is its top limb
    return r;
  }
  // a - 2 b + V p.  Needs 2 b <= V p.  Class: (class of a) + V.   Per limb in [-2^31, 2^31): a_i - 2 b_i + K_i + c with c in [-2, 1]
  template <int V>
  static PC_HD Fq30 sub_dbl(const Fq30& a, const Fq30& b) {
    constexpr L13 K = kp(V);
    Fq30 r; int32_t c = 0;
    PC_UNROLL for (int i = 0; i < N - 1; i++) {
      const int32_t t = (int32_t)(a.l[i] - 2u * b.l[i] + K.v[i]) + c;
      r.l[i] = (uint32_t)t & MASK; c = t >> 30;
    }
    r.l[N - 1] = a.l[N - 1] - 2u * b.l[N - 1] + K.v[N - 1] + (uint32_t)c;
    return r;
  }
  // V p - a.  Needs a <= V p.  Class V.
  template <int V>
  static PC_HD Fq30 neg(const Fq30& a) {
    constexpr L13 K = kp(V);
    Fq30 r; int32_t c = 0;
    PC_UNROLL for (int i = 0; i < N - 1; i++) {
      const int32_t t = (int32_t)(K.v[i] - a.l[i]) + c;
      r.l[i] = (uint32_t)t & MASK; c = t >> 30;
    }
    r.l[N - 1] = K.v[N - 1] - a.l[N - 1] + (uint32_t)c;
    return r;
  }
  // value = 0 (mod p), exact, for a value of class V: if it is q p then l[0] = q p_0 (mod 2^30), i.e. q = l[0] p^-1 mod 2^30, and
  // q <= V; only then (one value in 2^30 / V otherwise) are all limbs compared with those of q p
  template <int V>
  PC_HD bool is_zero_modp() const {
    const uint32_t q = (l[0] * PINV30) & MASK;
    if (q > (uint32_t)V) return false;
    constexpr L13 Pl = PL;
    uint64_t c = 0; uint32_t diff = 0;
    PC_UNROLL for (int i = 0; i < N - 1; i++) { c += (uint64_t)q * Pl.v[i]; diff |= l[i] ^ ((uint32_t)c & MASK); c >>= 30; }
    c += (uint64_t)q * Pl.v[N - 1];
    return diff == 0 && c == (uint64_t)l[N - 1];
  }

  template <int KIND, int VA, int VB, int VC, int VD>
  struct PlanOf { static constexpr Plan value = plan(KIND, VA, VB, VC, VD); };

  // ---- the multiplier by columns: the device's form.  PC_FQ30_HOST_COLUMNS compiles the same column code for the host with the
  // multiply-adds as plain 64-bit arithmetic, wrap-around included (tests/test_fq30_cpu.py runs the multiplier tests on both forms)
#if defined(__HIP_DEVICE_COMPILE__)
  // k partial products per asm statement, the carry-out of the 64-bit multiply-add discarded (the plan keeps every column below 2^64)
#define PC30_MAC1(A, B) "v_mad_u64_u32 %0, vcc, " A ", " B ", %0\n\t"
#define PC30_MAC_FNS(NAME, YC)                                                                                          \
  static __device__ __forceinline__ void NAME##1(uint64_t& acc, const uint32_t* x, const uint32_t* y) {                \
    asm(PC30_MAC1("%1", "%2") : "+v"(acc) : "v"(x[0]), YC(y[0]) : "vcc");                                               \
  }                                                                                                                     \
  static __device__ __forceinline__ void NAME##2(uint64_t& acc, const uint32_t* x, const uint32_t* y) {                \
    asm(PC30_MAC1("%1", "%2") PC30_MAC1("%3", "%4") : "+v"(acc) : "v"(x[0]), YC(y[0]), "v"(x[1]), YC(y[1]) : "vcc");    \
  }                                                                                                                     \
  static __device__ __forceinline__ void NAME##4(uint64_t& acc, const uint32_t* x, const uint32_t* y) {                \
    asm(PC30_MAC1("%1", "%2") PC30_MAC1("%3", "%4") PC30_MAC1("%5", "%6") PC30_MAC1("%7", "%8")                         \
        : "+v"(acc) : "v"(x[0]), YC(y[0]), "v"(x[1]), YC(y[1]), "v"(x[2]), YC(y[2]), "v"(x[3]), YC(y[3]) : "vcc");      \
  }                                                                                                                     \
  static __device__ __forceinline__ void NAME##8(uint64_t& acc, const uint32_t* x, const uint32_t* y) {                \
    asm(PC30_MAC1("%1", "%2") PC30_MAC1("%3", "%4") PC30_MAC1("%5", "%6") PC30_MAC1("%7", "%8")                         \
        PC30_MAC1("%9", "%10") PC30_MAC1("%11", "%12") PC30_MAC1("%13", "%14") PC30_MAC1("%15", "%16")                  \
        : "+v"(acc)                                                                                                     \
        : "v"(x[0]), YC(y[0]), "v"(x[1]), YC(y[1]), "v"(x[2]), YC(y[2]), "v"(x[3]), YC(y[3]),                           \
          "v"(x[4]), YC(y[4]), "v"(x[5]), YC(y[5]), "v"(x[6]), YC(y[6]), "v"(x[7]), YC(y[7]) : "vcc");                  \
  }
  PC30_MAC_FNS(mac, PC_Y_VGPR)
  PC30_MAC_FNS(macs, PC_Y_SGPR)      // second factor in a scalar register: the limbs of p
  template <int CNT>
  static __device__ __forceinline__ void mac_n(uint64_t& acc, const uint32_t* x, const uint32_t* y) {
    if constexpr (CNT >= 8) { mac8(acc, x, y); mac_n<CNT - 8>(acc, x + 8, y + 8); }
    else if constexpr (CNT >= 4) { mac4(acc, x, y); mac_n<CNT - 4>(acc, x + 4, y + 4); }
    else if constexpr (CNT >= 2) { mac2(acc, x, y); mac_n<CNT - 2>(acc, x + 2, y + 2); }
    else if constexpr (CNT == 1) mac1(acc, x, y);
  }
  template <int CNT>
  static __device__ __forceinline__ void mac_ns(uint64_t& acc, const uint32_t* x, const uint32_t* y) {
    if constexpr (CNT >= 8) { macs8(acc, x, y); mac_ns<CNT - 8>(acc, x + 8, y + 8); }
    else if constexpr (CNT >= 4) { macs4(acc, x, y); mac_ns<CNT - 4>(acc, x + 4, y + 4); }
    else if constexpr (CNT >= 2) { macs2(acc, x, y); mac_ns<CNT - 2>(acc, x + 2, y + 2); }
    else if constexpr (CNT == 1) macs1(acc, x, y);
  }
#elif defined(PC_FQ30_HOST_COLUMNS)
  template <int CNT> static inline void mac_n(uint64_t& acc, const uint32_t* x, const uint32_t* y) { for (int i = 0; i < CNT; i++) acc += (uint64_t)x[i] * y[i]; }
  template <int CNT> static inline void mac_ns(uint64_t& acc, const uint32_t* x, const uint32_t* y) { mac_n<CNT>(acc, x, y); }
  static inline void macs1(uint64_t& acc, const uint32_t* x, const uint32_t* y) { mac_n<1>(acc, x, y); }
#endif
#if defined(__HIP_DEVICE_COMPILE__) || defined(PC_FQ30_HOST_COLUMNS)
  static PC_D void set_aside(uint64_t& acc, uint64_t& aside) { aside += acc >> 32; acc &= 0xffffffffu; }
  // the products x_i y_{K-i} of column K
  template <int K>
  static PC_D void prod_terms(const uint32_t* x_, const uint32_t* y_, uint64_t& acc) {
    constexpr int I0 = K > N - 1 ? K - (N - 1) : 0, I1 = K < N - 1 ? K : N - 1, CNT = I1 - I0 + 1;
    uint32_t x[CNT], y[CNT];
    int c = 0;
    PC_UNROLL for (int i = I0; i <= I1; i++) { x[c] = x_[i]; y[c] = y_[K - i]; c++; }
    mac_n<CNT>(acc, x, y);
  }
  // the squaring's terms of column K: a_i (2 a_j) for i < j, i + j = K (d = 2 a limb by limb: limbs have the room), and a_{K/2}^2
  template <int K>
  static PC_D void sq_terms(const uint32_t* a, const uint32_t* d, uint64_t& acc) {
    constexpr int I0 = K > N - 1 ? K - (N - 1) : 0;
    constexpr int NC = (K + 1) / 2 - I0 > 0 ? (K + 1) / 2 - I0 : 0, DG = (K & 1) ? 0 : 1, CNT = NC + DG;
    uint32_t x[CNT], y[CNT];
    int c = 0;
    PC_UNROLL for (int i = I0; i < I0 + NC; i++) { x[c] = a[i]; y[c] = d[K - i]; c++; }
    if constexpr (DG) { x[c] = a[K / 2]; y[c] = a[K / 2]; c++; }
    mac_n<CNT>(acc, x, y);
  }
  // One column: its products, the reduction terms m_i p_{K-i}, then either the Montgomery factor m_K with its term m_K p_0 (K < 13: the
  // low 30 bits become zero) or the result limb K - 13; the accumulator moves on by 30 bits.  For SQR `b` is 2a.
  template <int KIND, int VA, int VB, int VC, int VD, int K>
  static PC_D void column(const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d, uint32_t* m,
                                                uint32_t* t, uint64_t& acc) {
    constexpr Plan pl = PlanOf<KIND, VA, VB, VC, VD>::value;
    constexpr bool ANY = pl.split[K][0] || pl.split[K][1] || pl.split[K][2];
    uint64_t aside = 0;
    if constexpr (pl.split[K][0]) set_aside(acc, aside);
    if constexpr (KIND == SQR) sq_terms<K>(a, b, acc); else prod_terms<K>(a, b, acc);
    if constexpr (KIND == DUAL) {
      if constexpr (pl.split[K][1]) set_aside(acc, aside);
      prod_terms<K>(c, d, acc);
    }
    if constexpr (pl.split[K][2]) set_aside(acc, aside);
    constexpr int I0 = K > N - 1 ? K - (N - 1) : 0, R1 = K < N ? K - 1 : N - 1, RC = R1 - I0 + 1;
    if constexpr (RC > 0) {
      constexpr L13 Pl = PL;
      uint32_t x[RC], y[RC];
      int n = 0;
      PC_UNROLL for (int i = I0; i <= R1; i++) { x[n] = m[i]; y[n] = Pl.v[K - i]; n++; }
      mac_ns<RC>(acc, x, y);
    }
    if constexpr (K < N) {
      m[K] = ((uint32_t)acc * INV30) & MASK;
      constexpr uint32_t p0c = kp(1).v[0];
      const uint32_t p0 = p0c;
      macs1(acc, &m[K], &p0);
    } else {
      t[K - N] = (uint32_t)acc & MASK;
    }
    acc >>= 30;
    if constexpr (ANY) acc += aside << 2;
    if constexpr (K + 1 < 2 * N - 1) column<KIND, VA, VB, VC, VD, K + 1>(a, b, c, d, m, t, acc);
  }
  template <int KIND, int VA, int VB, int VC, int VD>
  static PC_D Fq30 mont_cols(const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d) {
    uint32_t m[N], t[N];
    uint64_t acc = 0;
    column<KIND, VA, VB, VC, VD, 0>(a, b, c, d, m, t, acc);
    t[N - 1] = (uint32_t)acc;
    Fq30 r;
    PC_UNROLL for (int i = 0; i < N; i++) r.l[i] = t[i];
    return r;
  }
#endif
#if !defined(__HIP_DEVICE_COMPILE__)
  // host: (a b [+ c d] + m p)/R' by rows; every partial sum stays far below 2^64 (30-bit limbs, 34-bit carries)
  static inline Fq30 mont_rows_host(const Fq30& a, const Fq30& b, const Fq30* c, const Fq30* d) {
    uint64_t t[N + 1];
    for (int i = 0; i <= N; i++) t[i] = 0;
    for (int i = 0; i < N; i++) {
      for (int pass = 0; pass < (c ? 2 : 1); pass++) {
        const Fq30& x = pass ? *c : a; const uint64_t yi = pass ? d->l[i] : b.l[i];
        uint64_t cy = 0;
        for (int j = 0; j < N; j++) { cy += t[j] + (uint64_t)x.l[j] * yi; t[j] = cy & MASK; cy >>= 30; }
        t[N] += cy;
      }
      const uint64_t m = ((uint32_t)t[0] * INV30) & MASK;
      uint64_t cy = (t[0] + m * PL.v[0]) >> 30;
      for (int j = 1; j < N; j++) { cy += t[j] + m * PL.v[j]; t[j - 1] = cy & MASK; cy >>= 30; }
      t[N - 1] = cy + t[N]; t[N] = 0;          // (limb 12 holds the rest: it is re-cut by the next row)
    }
    Fq30 r;
    for (int i = 0; i < N; i++) r.l[i] = (uint32_t)t[i];
    return r;
  }
#endif

  // ---- the multiplier: (a b [+ c d] + m p) / R', no final subtraction.  Classes in, class mul_out(...) out ------------------
  template <int VA, int VB>
  static PC_HD Fq30 mul(const Fq30& a, const Fq30& b) {
    static_assert(PlanOf<MUL, VA, VB, 0, 0>::value.ok, "a column of the product does not fit its accumulator");
#if defined(__HIP_DEVICE_COMPILE__) || defined(PC_FQ30_HOST_COLUMNS)
    return mont_cols<MUL, VA, VB, 0, 0>(a.l, b.l, nullptr, nullptr);
#else
    return mont_rows_host(a, b, nullptr, nullptr);
#endif
  }
  // a^2: 91 products instead of 169 (cross terms once, against the doubled limbs)
  template <int VA>
  static PC_HD Fq30 sqr(const Fq30& a) {
    static_assert(PlanOf<SQR, VA, VA, 0, 0>::value.ok, "a column of the squaring does not fit its accumulator");
#if defined(__HIP_DEVICE_COMPILE__) || defined(PC_FQ30_HOST_COLUMNS)
    uint32_t d[N];
    PC_UNROLL for (int i = 0; i < N; i++) d[i] = a.l[i] << 1;
    return mont_cols<SQR, VA, VA, 0, 0>(a.l, d, nullptr, nullptr);
#else
    return mont_rows_host(a, a, nullptr, nullptr);
#endif
  }
  // a b + c d with one reduction: 3 * 169 products instead of 4 * 169
  template <int VA, int VB, int VC, int VD>
  static PC_HD Fq30 mul_add_mul(const Fq30& a, const Fq30& b, const Fq30& c, const Fq30& d) {
    static_assert(PlanOf<DUAL, VA, VB, VC, VD>::value.ok, "a column of the fused pair does not fit its accumulator");
#if defined(__HIP_DEVICE_COMPILE__) || defined(PC_FQ30_HOST_COLUMNS)
    return mont_cols<DUAL, VA, VB, VC, VD>(a.l, b.l, c.l, d.l);
#else
    return mont_rows_host(a, b, &c, &d);
#endif
  }
};

}  // namespace pc
