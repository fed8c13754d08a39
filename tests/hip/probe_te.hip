// TEST-ONLY probe unit: the twisted Edwards group law of ed_on_bls12_381 one primitive per lane, chains of mixed additions, and the
// product's own kernel bodies of csrc/te.hpp run as they are.  The adapters below only hand the bodies their (device) pointers;
// NafMasks and TeFoldDigits are made on the host and passed by value, one scalar per launch, as abi_te.hip does.
#include "probe_te_runner.hpp"
#include "probe_te_bodies.hpp"

namespace {
typedef pc::TeOf<pc_te_ed_on_bls12_381> TeC;
typedef pc::XyzzD<TeC> Pt;
typedef pc::AffD<TeC> Aff;
constexpr size_t XW = Pt::WORDS, AW = Aff::WORDS, XYW = Aff::XY_WORDS, FN = Pt::Fq::N;
constexpr int NW = TeC::FrP::N;
}  // namespace

// op = probe::TeOp; in: n x 64 words, out: n x (32 + 24)
extern "C" int pc_probe_te(int op, size_t n, const uint32_t* in, uint32_t* out) {
  return probe::dispatch<probe::TeBodies<TeC>::Body, probe::T_NOPS>(op, n, in, out);
}

// in: lanes x (1 + max_steps) words; table: 64 resident records; out: lanes x TeChainBody::OUT_WORDS
extern "C" int pc_probe_te_chain(size_t lanes, uint32_t max_steps, const uint32_t* in, const uint32_t* table, uint32_t* out) {
  typedef probe::TeChainBody<TeC> Body;
  return probe::Runner::run<Body>(lanes, in, lanes * (1 + (size_t)max_steps), out, lanes * Body::OUT_WORDS, table, 64 * AW, max_steps);
}

// ext[i] = key[i] + u key[half + i] by the ladder; key: 2 half resident records, u: the canonical scalar (8 words), ext: half x 32
extern "C" int pc_probe_te_ec_fold(size_t half, const uint32_t* key, const uint32_t* u, uint32_t* ext) {
  pc::NafMasks<NW> naf; naf.from_scalar(u);
  const probe::Buf bufs[] = {{key, nullptr, 2 * half * AW}, {nullptr, ext, half * XW}};
  return probe::run_bufs(half, bufs, 2, [&](uint32_t* const* d) {
    pc::TeEcFoldBody<TeC> f; f.key = d[0]; f.half = (uint32_t)half; f.ext = d[1]; f.naf = naf; return f;
  });
}

// the non-zero NAF digits of u as the table fold walks them: out = count | d[128]; PROBE_UNSUPPORTED where from_naf refuses
// (a digit at or above `rows`)
extern "C" int pc_probe_te_fold_digits(const uint32_t* u, uint32_t rows, uint32_t* out) {
  pc::NafMasks<NW> naf; naf.from_scalar(u);
  pc::TeFoldDigits dg;
  if (!dg.from_naf(naf, rows)) return PROBE_UNSUPPORTED;
  out[0] = dg.count;
  for (uint32_t k = 0; k < pc::TeFoldDigits::MAX; k++) out[1 + k] = k < dg.count ? dg.d[k] : 0;
  return 0;
}

// the same sums from the fold table; key: half resident records (the lower half), tbl: tbl_rows x half records of which the digits
// may use the first `rows`; PROBE_UNSUPPORTED (and no launch) where from_naf refuses
extern "C" int pc_probe_te_table_fold(size_t half, const uint32_t* key, const uint32_t* tbl, uint32_t tbl_rows, uint32_t rows, const uint32_t* u,
                                      uint32_t* ext) {
  if (rows > tbl_rows) return PROBE_BAD_OP;
  pc::NafMasks<NW> naf; naf.from_scalar(u);
  pc::TeFoldDigits dg;
  if (!dg.from_naf(naf, rows)) return PROBE_UNSUPPORTED;
  const probe::Buf bufs[] = {{key, nullptr, half * AW}, {tbl, nullptr, (size_t)tbl_rows * half * AW}, {nullptr, ext, half * XW}};
  return probe::run_bufs(half, bufs, 3, [&](uint32_t* const* d) {
    pc::TeTableFoldBody<TeC> t; t.key = d[0]; t.tbl = d[1]; t.half = (uint32_t)half; t.ext = d[2]; t.dg = dg; return t;
  });
}

// n extended points -> n resident records, one inversion per run of K
extern "C" int pc_probe_te_batch_affine(size_t n, uint32_t K, const uint32_t* ext, uint32_t* out) {
  if (K == 0) return PROBE_BAD_OP;
  const probe::Buf bufs[] = {{ext, nullptr, n * XW}, {nullptr, nullptr, n * FN}, {nullptr, out, n * AW}};
  return probe::run_bufs((n + K - 1) / K, bufs, 3, [&](uint32_t* const* d) {
    return pc::TeBatchAffineBody<TeC>{d[0], d[1], d[2], (uint32_t)n, K};
  });
}

// ext[j] = 2 in[j]: n resident records -> n x 32 extended words
extern "C" int pc_probe_te_dbl_row(size_t n, const uint32_t* in, uint32_t* ext) {
  const probe::Buf bufs[] = {{in, nullptr, n * AW}, {nullptr, ext, n * XW}};
  return probe::run_bufs(n, bufs, 2, [&](uint32_t* const* d) { return pc::TeDblRowBody<TeC>{d[0], d[1]}; });
}

// flags[i] = 1 if r key[i] is the identity
extern "C" int pc_probe_te_subgroup(size_t n, const uint32_t* key, uint32_t* flags) {
  pc::NafMasks<NW> naf; naf.from_scalar(TeC::FrP::MOD);
  const probe::Buf bufs[] = {{key, nullptr, n * AW}, {nullptr, flags, n}};
  return probe::run_bufs(n, bufs, 2, [&](uint32_t* const* d) {
    pc::TeSubgroupBody<TeC> b; b.key = d[0]; b.flags = d[1]; b.naf = naf; return b;
  });
}

// x | y -> x | y | td, and back
extern "C" int pc_probe_te_derive(size_t n, const uint32_t* xy, uint32_t* out) {
  const probe::Buf bufs[] = {{xy, nullptr, n * XYW}, {nullptr, out, n * AW}};
  return probe::run_bufs(n, bufs, 2, [&](uint32_t* const* d) { return pc::TeDeriveBody<TeC>{d[0], d[1]}; });
}
extern "C" int pc_probe_te_strip(size_t n, const uint32_t* in, uint32_t* out_xy) {
  const probe::Buf bufs[] = {{in, nullptr, n * AW}, {nullptr, out_xy, n * XYW}};
  return probe::run_bufs(n, bufs, 2, [&](uint32_t* const* d) { return pc::TeStripBody<TeC>{d[0], d[1]}; });
}
