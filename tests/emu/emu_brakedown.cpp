// Host compilation of csrc/sprs.hpp: the checks of pc_hip_brakedown_code_create as the library runs them, and one Brakedown encode
// with every kernel body stepped lane by lane in launch order (tests/test_brakedown_cpu.py).  Build: g++ -O2 -shared -fPIC.
#include <stdint.h>
#include <vector>
#include "../../poly_commit_amd/csrc/sprs.hpp"

struct CpuStepBackend {
  int marks = 0;
  template <class B> void launch(const B& body, size_t lanes) { for (size_t i = 0; i < lanes; i++) body((uint32_t)i); }
  void mark() { marks++; }
};

template <class FrP>
static int encode_t(const pc::BrakedownLayout& L, const size_t* ind_ptr, const uint32_t* col_ind, const uint32_t* val, const uint32_t* msgs,
                    uint32_t rows, uint32_t* out) {
  const pc::BrakedownImage im = pc::brakedown_image(L);
  std::vector<uint8_t> image(im.bytes + 32, 0);
  std::vector<uint32_t> pts((L.rsoe - L.rss) * 8 + 8);
  pc::brakedown_points<FrP>(pts.data(), L.rsoe - L.rss);
  pc::BrakedownDev D;
  pc::brakedown_fill(L, ind_ptr, col_ind, val, pts.data(), image.data(), image.data(), &D);
  // the working buffer starts out as garbage, as device memory does: every place that is read must have been written by the schedule
  std::vector<uint32_t> T((size_t)D.work_len() * rows * 8, 0xA5A5A5A5u);
  CpuStepBackend be;
  pc::brakedown_encode<FrP>(be, D, msgs, rows, T.data(), out);
  return be.marks == 2 ? 0 : -1;
}

extern "C" int emu_brakedown_validate(size_t msg_len, size_t codeword_len, size_t n_levels, const size_t* dims, const size_t* ind_ptr,
                                      const uint32_t* col_ind, size_t nnz) {
  return pc::brakedown_validate(msg_len, codeword_len, n_levels, dims, ind_ptr, col_ind, nnz, nullptr);
}

// field: 0 BLS12-381 Fr, 1 BN254 Fr, 2 Pallas Fr, 3 BLS12-377 Fr (pc_curve).  Returns the validation's answer; only a valid code is encoded.
extern "C" int emu_brakedown_encode(int field, size_t msg_len, size_t codeword_len, size_t n_levels, const size_t* dims, const size_t* ind_ptr,
                                    const uint32_t* col_ind, const uint32_t* val, size_t nnz, const uint32_t* msgs, uint32_t rows, uint32_t* out) {
  pc::BrakedownLayout L;
  const int rc = pc::brakedown_validate(msg_len, codeword_len, n_levels, dims, ind_ptr, col_ind, nnz, &L);
  if (rc) return rc;
  if (field == 0) return encode_t<pc_bls12_381_fr>(L, ind_ptr, col_ind, val, msgs, rows, out);
  if (field == 1) return encode_t<pc_bn254_fr>(L, ind_ptr, col_ind, val, msgs, rows, out);
  if (field == 3) return encode_t<pc_bls12_377_fr>(L, ind_ptr, col_ind, val, msgs, rows, out);
  return encode_t<pc_pallas_fr>(L, ind_ptr, col_ind, val, msgs, rows, out);
}
