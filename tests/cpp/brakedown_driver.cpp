// Test driver of the C++ host mirror of the Brakedown code (poly_commit_amd/host/brakedown.hpp); tests/test_brakedown_cpu.py and
// tests/test_brakedown_gpu.py compare what it prints and writes with the Python restatement (tests/harness/brakedown.py).
//   rowmul                                  the reference's test_sprs_row_mul vectors through both constructors (utils.rs:275-301)
//   table                                   default dimensions for num_vars 10..24 and both modulus bit sizes, one line each
//   makemat field n m d seed out            make_mat over Gen(seed): ind_ptr (u64 x m+1) | col_ind (u64 x nnz) | val (32 bytes x nnz)
//   encode field num_vars seed rows out     the default code over Gen(seed), `rows` messages from Gen(seed + 1), encoded on the HOST
//   time num_vars threads reps              BN254: milliseconds of the host encode of the scheme's n rows (median of reps)
//   device field num_vars seed              needs a GPU: pc_hip_brakedown_encode of the scheme's n rows against the host encode
//   pcs field num_vars seed out             needs a GPU: BrakedownPCS commit / open / check of the evaluations from Gen(seed + 1) at the point from
//                                           Gen(seed + 2), r from Gen(seed + 3), indices (i * 7919 + 13) % m_ext with the last column first;
//                                           out: root (32 bytes) | v | well-formedness vector
#include <algorithm>
#include <chrono>
#include <stdio.h>
#include <stdlib.h>
#include "../../poly_commit_amd/host/brakedown.hpp"
using namespace pc_host;

// the caller's RngCore of the tests: splitmix64; a field element is four draws (low word first) cut below the modulus' top bit
struct Gen {
  uint64_t s;
  explicit Gen(uint64_t seed) : s(seed) {}
  uint64_t next_u64() {
    s += 0x9E3779B97F4A7C15ull;
    uint64_t z = s;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
  template <class E> FrT<E> nonzero() {
    typedef typename FrT<E>::F F;
    for (;;) {
      F t; for (int i = 0; i < 4; i++) t.l[i] = next_u64();
      const int top = E::C::FrP::BITS - 1 - 192;
      t.l[3] &= (1ull << top) - 1;
      if (!(t.l[0] | t.l[1] | t.l[2] | t.l[3])) continue;
      F r2; memcpy(r2.l, E::C::FrP::R2, 32);
      return FrT<E>::of(t.mul(r2));
    }
  }
};

template <class E>
static int rowmul() {
  typedef FrT<E> Fr;
  const uint64_t flat[9] = {10, 23, 55, 100, 1, 58, 4, 0, 9}, v[3] = {12, 41, 55}, want[3] = {4088, 4431, 543};
  std::vector<Fr> list; for (uint64_t x : flat) list.push_back(Fr::from_u64(x));
  std::vector<std::vector<std::pair<size_t, Fr>>> cols(3);
  for (size_t j = 0; j < 3; j++) for (size_t i = 0; i < 3; i++) cols[j].push_back({i, list[3 * j + i]});
  Fr vv[3] = {Fr::from_u64(v[0]), Fr::from_u64(v[1]), Fr::from_u64(v[2])};
  auto a = SprsMat<E>::new_from_flat(3, 3, 3, list).row_mul(vv), b = SprsMat<E>::new_from_columns(3, 3, 3, cols).row_mul(vv);
  for (int i = 0; i < 3; i++) if (!(a[i] == Fr::from_u64(want[i])) || !(b[i] == a[i])) return 1;
  return 0;
}

static void print_dims(const std::vector<Dim>& d) { for (auto& x : d) printf(" %zu,%zu,%zu", std::get<0>(x), std::get<1>(x), std::get<2>(x)); }

template <class E>
static int makemat(size_t n, size_t m, size_t d, uint64_t seed, const char* path) {
  Gen g(seed);
  SprsMat<E> s = BrakedownPCParams<E>::make_mat(n, m, d, g);
  FILE* f = fopen(path, "wb"); if (!f) return 2;
  std::vector<uint64_t> a(s.ind_ptr.begin(), s.ind_ptr.end()), c(s.col_ind.begin(), s.col_ind.end());
  fwrite(a.data(), 8, a.size(), f); fwrite(c.data(), 8, c.size(), f); fwrite(s.val.data(), 32, s.val.size(), f);
  fclose(f);
  printf("nnz %zu\n", s.val.size());
  return 0;
}

template <class E>
static bool setup(size_t num_vars, uint64_t seed, size_t rows, BrakedownPCParams<E>& pp, Matrix<E>& mat) {
  Gen g(seed);
  if (!pp.make_default((size_t)1 << num_vars, g)) return false;
  Gen mg(seed + 1);
  mat.n = rows ? rows : pp.n; mat.m = pp.m; mat.entries.resize(mat.n * mat.m);
  for (auto& x : mat.entries) x = mg.nonzero<E>();
  return true;
}

template <class E>
static int encode(size_t num_vars, uint64_t seed, size_t rows, const char* path) {
  BrakedownPCParams<E> pp; Matrix<E> mat, ext;
  if (!setup(num_vars, seed, rows, pp, mat)) return 1;
  MultilinearBrakedown<E>::encode_rows_host(mat, pp, ext, 4);
  FILE* f = fopen(path, "wb"); if (!f) return 2;
  fwrite(ext.entries.data(), 32, ext.entries.size(), f); fclose(f);
  printf("rows %zu m %zu m_ext %zu\n", mat.n, pp.m, pp.m_ext);
  return 0;
}

template <class E>
static int device(size_t num_vars, uint64_t seed) {
  pc_ctx* ctx = nullptr;
  int rc = pc_hip_init(0, &ctx);
  if (rc != PC_OK) { printf("pc_hip_init failed: %s\n", pc_hip_strerror(rc)); return rc == PC_ERR_NO_DEVICE ? 77 : 1; }
  BrakedownPCParams<E> pp; Matrix<E> mat, want, got;
  if (!setup(num_vars, seed, 0, pp, mat)) return 1;
  pc_lincode* code = nullptr;
  int r = 1;
  if (Error e = pp.upload(ctx, &code)) printf("upload: %s\n", e.msg.c_str());
  else if (Error e2 = MultilinearBrakedown<E>::encode(ctx, code, mat, got)) printf("encode: %s\n", e2.msg.c_str());
  else {
    MultilinearBrakedown<E>::encode_rows_host(mat, pp, want, 16);
    r = (want.entries.size() == got.entries.size() && !memcmp(want.entries.data(), got.entries.data(), want.entries.size() * 32)) ? 0 : 1;
    printf(r ? "device encode differs from the host encode\n" : "device encode OK (%zu x %zu -> %zu, t = %ld)\n", mat.n, pp.m, pp.m_ext, pp.num_queries());
  }
  pc_hip_brakedown_code_free(code);
  pc_hip_shutdown(ctx);
  return r;
}

template <class E>
static int pcs(size_t num_vars, uint64_t seed, const char* path) {
  typedef FrT<E> Fr;
  pc_ctx* ctx = nullptr;
  int rc = pc_hip_init(0, &ctx);
  if (rc != PC_OK) { printf("pc_hip_init failed: %s\n", pc_hip_strerror(rc)); return rc == PC_ERR_NO_DEVICE ? 77 : 1; }
  BrakedownPCParams<E> pp;
  Gen g(seed), ge(seed + 1), gp(seed + 2), gr(seed + 3);
  if (!pp.make_default((size_t)1 << num_vars, g)) return 1;
  std::vector<Fr> evals((size_t)1 << num_vars), point(num_vars), r(pp.n);
  for (auto& x : evals) x = ge.nonzero<E>();
  for (auto& x : point) x = gp.nonzero<E>();
  for (auto& x : r) x = gr.nonzero<E>();
  const long t = pp.num_queries();
  std::vector<size_t> idx; for (long i = 0; i < t; i++) idx.push_back(((size_t)i * 7919 + 13) % pp.m_ext);
  idx[0] = pp.m_ext - 1;
  // the multilinear extension's value by folding one variable at a time (variable i is bit i of the index)
  std::vector<Fr> f = evals;
  for (size_t i = 0; i < num_vars; i++) { for (size_t j = 0; j < f.size() / 2; j++) f[j] = f[2 * j] + (f[2 * j + 1] - f[2 * j]) * point[i]; f.resize(f.size() / 2); }
  const Fr value = f[0];
  pc_lincode* code = nullptr;
  BrakedownPCS<E> S; LinCodePCCommitment com; LinCodePCCommitmentState<E> st; typename BrakedownPCS<E>::ProofSingle proof;
  int ret = 1; bool ok = false;
  auto fail = [&](const char* what, const Error& e) { printf("%s: kind %d %s\n", what, (int)e.kind, e.msg.c_str()); };
  do {
    if (Error e = pp.upload(ctx, &code)) { fail("upload", e); break; }
    if (Error e = S.commit(ctx, code, pp, evals, com, st)) { fail("commit", e); break; }
    if (Error e = S.open(ctx, com, st, point, idx, &r, proof)) { fail("open", e); break; }
    if (Error e = S.check(ctx, code, com, point, value, proof, idx, &r, ok)) { fail("check", e); break; }
    if (!ok) { printf("check rejected an honest proof\n"); break; }
    if (S.check(ctx, code, com, point, value + Fr::one(), proof, idx, &r, ok) || ok) { printf("check accepted a wrong value\n"); break; }
    { auto bad = proof; bad.columns[1][0] = bad.columns[1][0] + Fr::one();
      if (S.check(ctx, code, com, point, value, bad, idx, &r, ok).kind != Error::InvalidCommitment) { printf("altered column accepted\n"); break; } }
    { auto bad = proof; bad.paths[2][0] ^= 1;
      if (S.check(ctx, code, com, point, value, bad, idx, &r, ok).kind != Error::InvalidCommitment) { printf("altered path node accepted\n"); break; } }
    { auto bad = proof; bad.well_formedness[0] = bad.well_formedness[0] + Fr::one();
      if (S.check(ctx, code, com, point, value, bad, idx, &r, ok).kind != Error::InvalidCommitment) { printf("altered well-formedness vector accepted\n"); break; } }
    FILE* f2 = fopen(path, "wb"); if (!f2) break;
    fwrite(com.root, 1, 32, f2); fwrite(proof.v.data(), 32, proof.v.size(), f2); fwrite(proof.well_formedness.data(), 32, proof.well_formedness.size(), f2);
    fclose(f2);
    printf("brakedown commit/open/check OK (%zu x %zu -> %zu, t = %ld)\n", pp.n, pp.m, pp.m_ext, t);
    ret = 0;
  } while (0);
  pc_hip_brakedown_code_free(code);
  pc_hip_shutdown(ctx);
  return ret;
}

#define BY_FIELD(f, call) ((f) == 0 ? call<Bls12_381> : (f) == 1 ? call<Bn254> : call<Pallas>)

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "rowmul") {
    if (rowmul<Bls12_381>() || rowmul<Bn254>() || rowmul<Pallas>()) { printf("row_mul differs from the reference's vector\n"); return 1; }
    printf("rowmul OK\n");
    return 0;
  }
  if (mode == "table") {
    for (unsigned bits : {254u, 255u})
      for (size_t nv : {10, 12, 16, 20, 24}) {
        BrakedownPCParams<Bn254> pp;
        if (!pp.default_shape((size_t)1 << nv, bits)) return 1;
        printf("%u %zu %zu %zu %zu |", bits, nv, pp.n, pp.m, pp.m_ext); print_dims(pp.a_dims); printf(" |"); print_dims(pp.b_dims); printf("\n");
      }
    return 0;
  }
  if (mode == "makemat" && argc == 8)
    return BY_FIELD(atoi(argv[2]), makemat)(strtoull(argv[3], 0, 0), strtoull(argv[4], 0, 0), strtoull(argv[5], 0, 0), strtoull(argv[6], 0, 0), argv[7]);
  if (mode == "encode" && argc == 7)
    return BY_FIELD(atoi(argv[2]), encode)(strtoull(argv[3], 0, 0), strtoull(argv[4], 0, 0), strtoull(argv[5], 0, 0), argv[6]);
  if (mode == "device" && argc == 5)
    return BY_FIELD(atoi(argv[2]), device)(strtoull(argv[3], 0, 0), strtoull(argv[4], 0, 0));
  if (mode == "pcs" && argc == 6)
    return BY_FIELD(atoi(argv[2]), pcs)(strtoull(argv[3], 0, 0), strtoull(argv[4], 0, 0), argv[5]);
  if (mode == "time" && argc == 5) {
    BrakedownPCParams<Bn254> pp; Matrix<Bn254> mat, ext;
    if (!setup(strtoull(argv[2], 0, 0), 1, 0, pp, mat)) return 1;
    const unsigned threads = (unsigned)atoi(argv[3]); const int reps = atoi(argv[4]);
    std::vector<double> ms;
    for (int i = 0; i < reps; i++) {
      const auto t0 = std::chrono::steady_clock::now();
      MultilinearBrakedown<Bn254>::encode_rows_host(mat, pp, ext, threads);
      ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    std::sort(ms.begin(), ms.end());
    printf("host_encode_ms %.3f rows %zu m %zu m_ext %zu threads %u\n", ms[ms.size() / 2], mat.n, pp.m, pp.m_ext, threads);
    return 0;
  }
  printf("usage: brakedown_driver rowmul | table | makemat field n m d seed out | encode field num_vars seed rows out | time num_vars threads reps | device field num_vars seed | pcs field num_vars seed out\n");
  return 2;
}
