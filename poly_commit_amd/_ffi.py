"""ctypes binding of include/pc_hip.h.  No fallbacks: if the HIP library is missing or no
GPU is present, construction fails loudly."""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CURVES = {"bls12_381": 0, "bn254": 1, "pallas": 2, "bls12_377": 3}
FQ_BYTES = {"bls12_381": 48, "bn254": 32, "pallas": 32, "bls12_377": 48}
# the twisted Edwards curves (pc_te_curve): an id space of their own, with typed keys and entry points of their own
TE_CURVES = {"ed_on_bls12_381": 0}
TE_POINT_BYTES = {"ed_on_bls12_381": 64}
PC_MEM_HOST, PC_MEM_DEVICE = 0, 1
PC_SCALARS_CANONICAL, PC_SCALARS_MONTGOMERY = 0, 1

_lib = None


class PcHipError(RuntimeError):
    def __init__(self, status, msg=""):
        super().__init__(f"pc_hip status {status}: {msg}")
        self.status = status


def library_path():
    # PC_HIP_LIB: alternative build of the same library (kernel tuning experiments)
    return os.environ.get("PC_HIP_LIB") or os.path.join(HERE, "libpc_hip.so")


def load_library():
    """Load libpc_hip.so (built by poly_commit_amd/build.py).  Raises if it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    # The PyTorch wheel bundles its own ROCm runtime; if libpc_hip.so pulls in the system
    # libamdhip64 first, torch later finds "No HIP GPUs".  Let torch bring its runtime up first
    # (harness concern only -- a Rust/C++ consumer links one runtime).
    try:
        import torch
        if torch.cuda.is_available():
            torch.cuda.init()
    except ImportError:
        pass
    path = library_path()
    if not os.path.exists(path):
        raise PcHipError(-100, f"{path} not built: run python -m poly_commit_amd.build "
                               "(or __graft_entry__.build())")
    lib = C.CDLL(path)
    vp, sz, ip = C.c_void_p, C.c_size_t, C.c_int
    lib.pc_hip_device_count.restype = ip
    lib.pc_hip_init.argtypes = [ip, C.POINTER(vp)]
    lib.pc_hip_shutdown.argtypes = [vp]
    lib.pc_hip_shutdown.restype = None
    lib.pc_hip_strerror.argtypes = [ip]
    lib.pc_hip_strerror.restype = C.c_char_p
    lib.pc_hip_last_error.argtypes = [vp]
    lib.pc_hip_last_error.restype = C.c_char_p
    lib.pc_hip_srs_upload.argtypes = [vp, ip, vp, sz, sz, ip, C.POINTER(vp)]
    lib.pc_hip_srs_load_serialized.argtypes = [vp, ip, vp, sz, ip, sz, C.POINTER(vp), C.POINTER(sz), C.POINTER(sz)]
    lib.pc_hip_srs_serialize.argtypes = [vp, vp, sz, sz, ip, vp, sz, C.POINTER(sz)]
    lib.pc_hip_universal_params_layout.argtypes = [ip, vp, sz, ip, C.POINTER(sz)]
    lib.pc_hip_srs_free.argtypes = [vp]
    lib.pc_hip_srs_precompute.argtypes = [vp, vp, C.c_uint, sz]
    lib.pc_hip_srs_free.restype = None
    lib.pc_hip_srs_len.argtypes = [vp]
    lib.pc_hip_srs_len.restype = sz
    lib.pc_hip_srs_device_ptr.argtypes = [vp]
    lib.pc_hip_srs_device_ptr.restype = vp
    lib.pc_hip_msm.argtypes = [vp, vp, sz, vp, ip, ip, sz, vp, C.POINTER(ip)]
    lib.pc_hip_msm_batch.argtypes = [vp, vp, C.POINTER(sz), C.POINTER(vp), C.POINTER(sz), sz, ip, ip, vp,
                                     C.POINTER(ip)]
    lib.pc_hip_malloc.argtypes = [vp, sz, C.POINTER(vp)]
    lib.pc_hip_free.argtypes = [vp, vp]
    lib.pc_hip_memcpy_h2d.argtypes = [vp, vp, vp, sz]
    lib.pc_hip_memcpy_d2h.argtypes = [vp, vp, vp, sz]
    lib.pc_hip_msm_many.argtypes = [vp, vp, sz, vp, ip, ip, sz, sz, vp, C.POINTER(ip)]
    lib.pc_hip_msm_async.argtypes = [vp, vp, sz, vp, ip, ip, sz, vp, C.POINTER(ip), C.POINTER(vp)]
    lib.pc_hip_job_wait.argtypes = [vp, vp]
    lib.pc_hip_set_msm_tuning.argtypes = [vp, C.c_uint, C.c_uint]
    lib.pc_hip_set_timing.argtypes = [vp, ip]
    lib.pc_hip_srs_precompute_ex.argtypes = [vp, vp, C.c_uint, sz, C.c_uint]
    lib.pc_hip_srs_bytes_resident.argtypes = [vp, C.POINTER(sz)]
    lib.pc_hip_ctx_bytes_resident.argtypes = [vp, C.POINTER(sz)]
    lib.pc_hip_ctx_trim.argtypes = [vp]
    lib.pc_hip_last_msm_phases_ms.argtypes = [vp, C.POINTER(C.c_float)]
    lib.pc_hip_last_msm_marks_ms.argtypes = [vp, C.POINTER(C.c_float)]
    lib.pc_hip_last_msm_shape.argtypes = [vp, C.POINTER(C.c_uint32)]
    lib.pc_hip_matrix_columns.argtypes = [vp, vp, sz, sz, vp, sz, vp, ip]
    lib.pc_hip_ntt_batch.argtypes = [vp, ip, vp, ip, sz, sz, C.c_uint, vp, ip]
    lib.pc_hip_last_ntt_phases_ms.argtypes = [vp, C.POINTER(C.c_float)]
    lib.pc_hip_witness_poly.argtypes = [vp, ip, vp, ip, sz, vp, vp, ip]
    lib.pc_hip_kzg_open.argtypes = [vp, vp, sz, vp, ip, sz, vp, vp, C.POINTER(C.c_int)]
    lib.pc_hip_column_hash.argtypes = [vp, ip, vp, ip, sz, sz, ip, vp, ip]
    lib.pc_hip_column_hash_part.argtypes = [vp, ip, ip, vp, sz, sz, sz, sz, sz, ip, ip, vp, vp]
    lib.pc_hip_merkle_tree.argtypes = [vp, ip, vp, ip, sz, ip, vp, ip]
    lib.pc_hip_ligero_commit.argtypes = [vp, ip, vp, ip, sz, sz, C.c_uint, ip, ip, ip, vp, ip, vp, vp]
    lib.pc_hip_last_ligero_phases_ms.argtypes = [vp, C.POINTER(C.c_float)]
    lib.pc_hip_brakedown_code_create.argtypes = [vp, ip, sz, sz, sz, vp, vp, vp, vp, sz, C.POINTER(vp)]
    lib.pc_hip_brakedown_code_free.argtypes = [vp]
    lib.pc_hip_brakedown_code_free.restype = None
    lib.pc_hip_brakedown_codeword_len.argtypes = [vp]
    lib.pc_hip_brakedown_codeword_len.restype = sz
    lib.pc_hip_brakedown_encode.argtypes = [vp, vp, vp, ip, sz, vp, ip]
    lib.pc_hip_brakedown_commit.argtypes = [vp, vp, vp, ip, sz, ip, ip, ip, vp, ip, vp, vp]
    lib.pc_hip_last_brakedown_phases_ms.argtypes = [vp, C.POINTER(C.c_float)]
    lib.pc_hip_fr_lincomb.argtypes = [vp, ip, C.POINTER(vp), ip, C.POINTER(sz), sz, vp, vp, ip, sz]
    lib.pc_hip_fr_fold.argtypes = [vp, ip, vp, vp, sz, vp]
    lib.pc_hip_fr_dot.argtypes = [vp, ip, vp, vp, sz, vp]
    lib.pc_hip_ipa_fold_dots.argtypes = [vp, ip, vp, vp, sz, vp, vp, vp]
    lib.pc_hip_fr_powers.argtypes = [vp, ip, vp, sz, vp]
    lib.pc_hip_ec_fold.argtypes = [vp, vp, sz, vp]
    lib.pc_hip_ec_fold_from.argtypes = [vp, vp, sz, vp, C.POINTER(vp)]
    lib.pc_hip_srs_precompute_fold.argtypes = [vp, vp]
    lib.pc_hip_srs_precompute_fold_ex.argtypes = [vp, vp, C.c_uint, C.c_uint]
    lib.pc_hip_srs_fold_table_info.argtypes = [vp, C.POINTER(C.c_uint), C.POINTER(C.c_uint)]
    lib.pc_hip_ec_fold2_from.argtypes = [vp, vp, sz, vp, vp, C.POINTER(vp)]
    lib.pc_hip_ipa_round2_msms.argtypes = [vp, vp, vp, sz, vp, vp, C.POINTER(ip), vp, C.POINTER(ip)]
    lib.pc_hip_ipa_open_rounds.argtypes = [vp, vp, vp, sz, vp, vp, IPA_CHALLENGE_FN, vp, sz, vp, vp, vp, vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    lib.pc_hip_ipa_key_scalars.argtypes = [vp, ip, vp, sz, vp, sz, vp, sz, vp, vp]
    lib.pc_hip_srs_read.argtypes = [vp, vp, sz, sz, vp]
    lib.pc_hip_fixed_base_batch_mul.argtypes = [vp, ip, vp, vp, sz, vp]
    lib.pc_hip_poly_eval.argtypes = [vp, ip, vp, ip, sz, vp, vp]
    lib.pc_hip_poly_div_scan.argtypes = [vp, ip, vp, ip, sz, vp, vp, vp, ip]
    lib.pc_hip_points_sum.argtypes = [ip, vp, sz, vp]
    lib.pc_hip_point_mul.argtypes = [ip, vp, vp, vp]
    lib.pc_hip_group_create.argtypes = [C.POINTER(ip), ip, C.POINTER(vp)]
    lib.pc_hip_group_destroy.argtypes = [vp]
    lib.pc_hip_group_destroy.restype = None
    lib.pc_hip_group_size.argtypes = [vp]
    lib.pc_hip_group_ctx.argtypes = [vp, ip]
    lib.pc_hip_group_ctx.restype = vp
    lib.pc_hip_group_srs_upload.argtypes = [vp, ip, vp, sz, sz, ip, C.POINTER(vp)]
    lib.pc_hip_group_srs_free.argtypes = [vp]
    lib.pc_hip_group_srs_free.restype = None
    lib.pc_hip_group_srs_len.argtypes = [vp]
    lib.pc_hip_group_srs_len.restype = sz
    lib.pc_hip_group_msm.argtypes = [vp, vp, sz, vp, ip, sz, vp, C.POINTER(ip)]
    lib.pc_hip_group_msm_batch.argtypes = [vp, vp, C.POINTER(vp), C.POINTER(sz), sz, ip, vp, C.POINTER(ip)]
    lib.pc_hip_group_kzg_open.argtypes = [vp, vp, vp, sz, vp, vp, C.POINTER(ip), vp]
    lib.pc_hip_group_ntt_batch.argtypes = [vp, ip, vp, sz, sz, C.c_uint, vp]
    lib.pc_hip_group_ligero_commit.argtypes = [vp, ip, vp, sz, sz, C.c_uint, ip, ip, ip, vp, vp, vp]
    lib.pc_hip_group_commit_open_async.argtypes = [vp, vp, vp, ip, sz, vp, vp, vp, vp, C.POINTER(vp)]
    lib.pc_hip_group_job_wait.argtypes = [vp, vp]
    lib.pc_hip_g2_srs_upload.argtypes = [vp, ip, vp, sz, sz, ip, C.POINTER(vp)]
    lib.pc_hip_g2_srs_free.argtypes = [vp]
    lib.pc_hip_g2_srs_free.restype = None
    lib.pc_hip_g2_srs_len.argtypes = [vp]
    lib.pc_hip_g2_srs_len.restype = sz
    lib.pc_hip_g2_srs_bytes_resident.argtypes = [vp, C.POINTER(sz)]
    lib.pc_hip_g2_srs_pair_sums.argtypes = [vp, vp, sz, sz, vp, sz]
    lib.pc_hip_g2_srs_read.argtypes = [vp, vp, sz, sz, vp]
    lib.pc_hip_g2_msm.argtypes = [vp, vp, sz, vp, ip, ip, sz, vp, C.POINTER(ip)]
    lib.pc_hip_g2_points_sum.argtypes = [ip, vp, sz, vp]
    lib.pc_hip_g2_point_mul.argtypes = [ip, vp, vp, vp]
    lib.pc_hip_te_srs_upload.argtypes = [vp, ip, vp, sz, sz, ip, C.POINTER(vp)]
    lib.pc_hip_te_srs_free.argtypes = [vp]
    lib.pc_hip_te_srs_free.restype = None
    lib.pc_hip_te_srs_len.argtypes = [vp]
    lib.pc_hip_te_srs_len.restype = sz
    lib.pc_hip_te_srs_read.argtypes = [vp, vp, sz, sz, vp]
    lib.pc_hip_te_srs_bytes_resident.argtypes = [vp, C.POINTER(sz)]
    lib.pc_hip_te_msm.argtypes = [vp, vp, sz, vp, ip, ip, sz, vp, C.POINTER(ip)]
    lib.pc_hip_te_msm_many.argtypes = [vp, vp, sz, vp, ip, ip, sz, sz, vp, C.POINTER(ip)]
    lib.pc_hip_te_fr_lincomb.argtypes = [vp, ip, C.POINTER(vp), ip, C.POINTER(sz), sz, vp, vp, ip, sz]
    lib.pc_hip_te_fr_dot.argtypes = [vp, ip, vp, vp, sz, vp]
    lib.pc_hip_te_ec_fold.argtypes = [vp, vp, sz, vp]
    lib.pc_hip_te_ec_fold_from.argtypes = [vp, vp, sz, vp, C.POINTER(vp)]
    lib.pc_hip_te_srs_precompute_fold.argtypes = [vp, vp]
    lib.pc_hip_te_srs_fold_table_info.argtypes = [vp, C.POINTER(C.c_uint)]
    lib.pc_hip_te_srs_in_subgroup.argtypes = [vp, vp, C.POINTER(ip)]
    lib.pc_hip_te_fr_powers.argtypes = [vp, ip, vp, sz, vp]
    lib.pc_hip_te_ipa_fold_dots.argtypes = [vp, ip, vp, vp, sz, vp, vp, vp]
    lib.pc_hip_te_ipa_key_scalars.argtypes = [vp, ip, vp, sz, vp, sz, vp, sz, vp, vp]
    lib.pc_hip_te_ipa_open_rounds.argtypes = [vp, vp, vp, sz, vp, vp, IPA_CHALLENGE_FN, vp, sz, vp, vp, vp, vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    lib.pc_hip_te_points_sum.argtypes = [ip, vp, sz, vp]
    lib.pc_hip_te_point_mul.argtypes = [ip, vp, vp, vp]
    lib.pc_hip_te_sample_generators.argtypes = [vp, ip, vp, sz, C.c_uint64, sz, C.POINTER(C.c_uint32), C.POINTER(vp)]
    lib.pc_hip_te_srs_prefix.argtypes = [vp, vp, sz, C.POINTER(vp)]
    lib.pc_hip_sample_generators.argtypes = [vp, ip, vp, sz, C.c_uint64, sz, C.POINTER(C.c_uint32), C.POINTER(vp)]
    lib.pc_hip_srs_prefix.argtypes = [vp, vp, sz, C.POINTER(vp)]
    lib.pc_hip_srs_check.argtypes = [vp, vp, sz, sz, C.c_uint, C.POINTER(sz), C.POINTER(sz), vp]
    lib.pc_hip_srs_in_subgroup.argtypes = [vp, vp, C.POINTER(ip)]
    lib.pc_hip_srs_load_serialized_ex.argtypes = [vp, ip, vp, sz, ip, sz, C.c_uint, C.POINTER(vp), C.POINTER(sz), C.POINTER(sz)]
    lib.pc_hip_g2_srs_check.argtypes = [vp, vp, sz, sz, C.c_uint, C.POINTER(sz), C.POINTER(sz), vp]
    lib.pc_hip_ml_fold.argtypes = [vp, ip, vp, sz, vp, vp, vp]
    lib.pc_hip_ml_open.argtypes = [vp, vp, vp, ip, C.c_uint, vp, vp, C.POINTER(ip)]
    lib.pc_hip_ml_eq_evals.argtypes = [vp, ip, vp, C.c_uint, vp]
    lib.pc_hip_g2_fixed_base_batch_mul.argtypes = [vp, ip, vp, vp, sz, vp]
    lib.pc_hip_g2_srs_device_ptr.argtypes = [vp]
    lib.pc_hip_g2_srs_device_ptr.restype = vp
    lib.pc_hip_ml_setup.argtypes = [vp, ip, C.c_uint, vp, vp, vp, C.POINTER(vp), C.POINTER(vp), vp]
    lib.pc_hip_ml_trim.argtypes = [vp, vp, vp, C.c_uint, C.c_uint, C.POINTER(vp), C.POINTER(vp)]
    lib.pc_hip_fold_tree.argtypes = [vp, ip, vp, ip, sz, vp, sz, vp, sz, C.POINTER(sz)]
    lib.pc_hip_poly_div_multi.argtypes = [vp, ip, vp, ip, sz, vp, sz, vp, ip, vp]
    lib.pc_hip_kzg_open_multi.argtypes = [vp, vp, sz, vp, ip, sz, vp, sz, vp, vp, C.POINTER(C.c_int)]
    lib.pc_hip_kzg_batch_open_multi.argtypes = [vp, vp, sz, C.POINTER(vp), ip, C.POINTER(sz), sz, vp, sz, vp, vp, C.POINTER(C.c_int)]
    lib.pc_hip_kzg_commit_folding.argtypes = [vp, vp, sz, vp, ip, sz, vp, sz, vp, C.POINTER(C.c_int)]
    lib.pc_hip_kzg_open_folding.argtypes = [vp, vp, sz, vp, ip, sz, vp, sz, vp, sz, vp, vp, vp, C.POINTER(C.c_int)]
    lib.pc_hip_last_skzg_launches.argtypes = [vp, C.POINTER(C.c_uint)]
    lib.pc_hip_pst13_key_len.argtypes = [sz, sz]
    lib.pc_hip_pst13_key_len.restype = sz
    lib.pc_hip_pst13_rank.argtypes = [sz, sz, vp, sz, vp]
    lib.pc_hip_pst13_unrank.argtypes = [sz, sz, vp, sz, vp]
    lib.pc_hip_pst13_monomial_evals.argtypes = [vp, ip, sz, sz, vp, vp]
    lib.pc_hip_pst13_scatter.argtypes = [vp, ip, sz, sz, vp, vp, ip, sz, vp]
    lib.pc_hip_pst13_divide.argtypes = [vp, ip, sz, sz, vp, ip, vp, vp, sz, C.POINTER(sz), vp]
    lib.pc_hip_pst13_commit.argtypes = [vp, vp, sz, sz, sz, vp, ip, vp, vp, ip, sz, vp, C.POINTER(C.c_int)]
    lib.pc_hip_pst13_open.argtypes = [vp, vp, sz, sz, sz, vp, ip, vp, vp, ip, sz, vp, vp, C.POINTER(C.c_int), vp]
    lib.pc_hip_pst13_trim.argtypes = [vp, vp, sz, sz, sz, sz, C.POINTER(vp)]
    lib.pc_hip_last_pst13_shape.argtypes = [vp, C.POINTER(C.c_uint32)]
    _lib = lib
    return lib


# pc_ipa_challenge_fn: void (*)(void* user, const void* l_xy, const void* r_xy, void* out_u_mont)
IPA_CHALLENGE_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)


def _ptr(x):
    """host numpy array -> (void*, PC_MEM_HOST); torch cuda tensor / int -> (void*, PC_MEM_DEVICE)."""
    if isinstance(x, np.ndarray):
        assert x.flags["C_CONTIGUOUS"]
        return C.c_void_p(x.ctypes.data), PC_MEM_HOST
    if isinstance(x, int):
        return C.c_void_p(x), PC_MEM_DEVICE
    if hasattr(x, "data_ptr"):   # torch tensor
        assert x.is_contiguous()
        return C.c_void_p(x.data_ptr()), (PC_MEM_DEVICE if x.is_cuda else PC_MEM_HOST)
    raise TypeError(type(x))


PST13_MAX_VARS = 32


def pst13_key_len(num_vars, degree):
    """M = C(num_vars + degree, num_vars), the length of a MarlinPST13 key in device order; 0 beyond the limits (pc_hip_pst13_key_len)"""
    return int(load_library().pc_hip_pst13_key_len(num_vars, degree))


def pst13_rank(num_vars, degree, exps):
    """device-order ranks of exponent tuples: exps (count, num_vars) uint8 -> (count,) uint32 (pc_hip_pst13_rank)"""
    lib = load_library()
    e = np.ascontiguousarray(exps, dtype=np.uint8).reshape(-1, num_vars)
    out = np.zeros(e.shape[0], dtype=np.uint32)
    rc = lib.pc_hip_pst13_rank(num_vars, degree, C.c_void_p(e.ctypes.data), e.shape[0], C.c_void_p(out.ctypes.data))
    if rc != 0:
        raise PcHipError(rc, lib.pc_hip_strerror(rc).decode())
    return out


def pst13_unrank(num_vars, degree, ranks):
    """the inverse: ranks (count,) -> (count, num_vars) uint8 (pc_hip_pst13_unrank)"""
    lib = load_library()
    r = np.ascontiguousarray(ranks, dtype=np.uint32).reshape(-1)
    out = np.zeros((r.shape[0], num_vars), dtype=np.uint8)
    rc = lib.pc_hip_pst13_unrank(num_vars, degree, C.c_void_p(r.ctypes.data), r.shape[0], C.c_void_p(out.ctypes.data))
    if rc != 0:
        raise PcHipError(rc, lib.pc_hip_strerror(rc).decode())
    return out


def _pst13_terms(num_vars, exps, coeffs, n_terms):
    """(exps pointer, coeffs pointer, where, count, what must stay alive across the call) of a term list: host arrays ((T, n) uint8 and
    (T, 4) uint64) or two device pointers with n_terms"""
    if exps is None:
        return None, None, PC_MEM_HOST, 0, None
    if isinstance(exps, np.ndarray) or isinstance(exps, (list, tuple)):
        e = np.ascontiguousarray(exps, dtype=np.uint8).reshape(-1, num_vars)
        c = np.ascontiguousarray(coeffs, dtype=np.uint64).reshape(-1, 4)
        assert e.shape[0] == c.shape[0]
        if not e.shape[0]:
            return None, None, PC_MEM_HOST, 0, None
        return C.c_void_p(e.ctypes.data), C.c_void_p(c.ctypes.data), PC_MEM_HOST, e.shape[0], (e, c)
    pe, we = _ptr(exps)
    pc_, wc = _ptr(coeffs)
    assert we == wc == PC_MEM_DEVICE and n_terms is not None
    return pe, pc_, PC_MEM_DEVICE, n_terms, None


class Context:
    """One GPU (pc_ctx)."""

    def __init__(self, device_id=0):
        self.lib = load_library()
        h = C.c_void_p()
        rc = self.lib.pc_hip_init(device_id, C.byref(h))
        if rc != 0:
            raise PcHipError(rc, self.lib.pc_hip_strerror(rc).decode())
        self.h = h
        self.device_id = device_id

    def check(self, rc):
        if rc != 0:
            raise PcHipError(rc, self.lib.pc_hip_strerror(rc).decode() + " / " +
                             self.lib.pc_hip_last_error(self.h).decode())

    def close(self):
        if self.h:
            self.lib.pc_hip_shutdown(self.h)
            self.h = None

    def set_msm_tuning(self, window_bits=0, chunk=0):
        self.check(self.lib.pc_hip_set_msm_tuning(self.h, window_bits, chunk))

    def set_timing(self, on=True):
        self.check(self.lib.pc_hip_set_timing(self.h, 1 if on else 0))

    def last_msm_phases_ms(self):
        out = (C.c_float * 8)()
        self.check(self.lib.pc_hip_last_msm_phases_ms(self.h, out))
        return list(out)

    def last_msm_marks_ms(self):
        """Phase boundaries of the last completed MSM as offsets from the last set_timing(True) (pc_hip_last_msm_marks_ms)."""
        out = (C.c_float * 8)()
        self.check(self.lib.pc_hip_last_msm_marks_ms(self.h, out))
        return list(out)

    def last_msm_shape(self):
        """{window bits, signed digits per scalar, buckets, window table used} of the last completed MSM."""
        out = (C.c_uint32 * 4)()
        self.check(self.lib.pc_hip_last_msm_shape(self.h, out))
        return {"window_bits": out[0], "digits_per_scalar": out[1], "buckets": out[2], "window_table": bool(out[3])}

    def ntt_batch(self, curve, mat, log_n, out=None, rows=None, in_cols=None):
        """rows x in_cols Fr (Montgomery) -> rows x 2^log_n, natural order.  numpy in -> numpy out;
        torch cuda tensors (or raw device pointers with rows/in_cols) stay on the device."""
        pin, win = _ptr(mat)
        if rows is None:
            rows, in_cols = mat.shape[0], mat.shape[1]
        if out is None:
            assert win == PC_MEM_HOST
            out = np.zeros((rows, 1 << log_n, 4), dtype=np.uint64)
        pout, wout = _ptr(out)
        self.check(self.lib.pc_hip_ntt_batch(self.h, CURVES[curve], pin, win, rows, in_cols, log_n, pout, wout))
        return out

    def column_hash(self, curve, ext, hash_name="blake2s", out=None, rows=None, n_cols=None):
        """Digests of the columns of the encoded matrix (rows x n_cols x Fr, Montgomery):
        FieldToBytesColHasher<F, D>, D = 'sha256' | 'blake2s'.  Returns (n_cols, 32) uint8 for host
        input; device buffers (raw pointers + rows/n_cols, out = device pointer) stay on the device."""
        pin, win = _ptr(ext)
        if rows is None:
            rows, n_cols = ext.shape[0], ext.shape[1]
        if out is None:
            assert win == PC_MEM_HOST
            out = np.zeros((n_cols, 32), dtype=np.uint8)
        pout, wout = _ptr(out)
        hid = {"sha256": 0, "blake2s": 1}[hash_name]
        self.check(self.lib.pc_hip_column_hash(self.h, CURVES[curve], pin, win, rows, n_cols, hid, pout, wout))
        return out

    def column_hash_part(self, curve, slab_dev, rows, n_cols, rows_total, state_dev, first, last, out_dev=0, hash_name="blake2s",
                         col0=0, cols=None):
        """One slab of rows absorbed into the per-column chaining states (pc_hip_column_hash_part): device pointers only.
        state_dev: n_cols x 48 bytes; out_dev: n_cols x 32 bytes, written when `last`."""
        hid = {"sha256": 0, "blake2s": 1}[hash_name]
        self.check(self.lib.pc_hip_column_hash_part(self.h, CURVES[curve], hid, C.c_void_p(slab_dev), rows, n_cols, rows_total, col0,
                                                    n_cols - col0 if cols is None else cols, 1 if first else 0, 1 if last else 0,
                                                    C.c_void_p(state_dev), C.c_void_p(out_dev)))

    def matrix_columns(self, mat_dev, rows, n_cols, indices):
        """Columns `indices` of a resident rows x n_cols matrix of 32-byte elements -> (t, rows, 4) uint64 host array."""
        idx = np.ascontiguousarray(indices, dtype=np.uint32)
        out = np.zeros((len(idx), rows, 4), dtype=np.uint64)
        self.check(self.lib.pc_hip_matrix_columns(self.h, mat_dev, rows, n_cols, idx.ctypes.data, len(idx), out.ctypes.data, PC_MEM_HOST))
        return out

    def merkle_tree(self, digests, hash_name="sha256", len_prefix=True, out=None, n_leaves=None):
        """Inner nodes of the Merkle tree over 32-byte leaf digests (create_merkle_tree,
        linear_codes/mod.rs:506-521), heap order, root at row 0: (2^h - 1, 32) uint8 for host input;
        device pointers (n_leaves given, out = device pointer) stay on the device."""
        pin, win = _ptr(digests)
        if n_leaves is None:
            n_leaves = digests.shape[0]
        h = max(1, (n_leaves - 1).bit_length())
        if out is None:
            assert win == PC_MEM_HOST
            out = np.zeros(((1 << h) - 1, 32), dtype=np.uint8)
        pout, wout = _ptr(out)
        hid = {"sha256": 0, "blake2s": 1}[hash_name]
        self.check(self.lib.pc_hip_merkle_tree(self.h, hid, pin, win, n_leaves, 1 if len_prefix else 0, pout, wout))
        return out

    def fr_lincomb(self, curve, polys, xi, n_out=None, out=None, lens=None):
        """sum_j xi[j] * polys[j] (MarlinKZG10::open's combination, marlin_pc/mod.rs:281-287).
        polys: list of (len_j, 4) uint64 host arrays, or device pointers with `lens`; xi: (k, 4)."""
        k = len(polys)
        ptrs = [_ptr(p) for p in polys]
        where = ptrs[0][1] if k else PC_MEM_HOST
        assert all(w == where for _, w in ptrs)
        if lens is None:
            lens = [p.shape[0] for p in polys]
        if n_out is None:
            n_out = max(lens) if k else 0
        if out is None:
            assert where == PC_MEM_HOST
            out = np.zeros((n_out, 4), dtype=np.uint64)
        pout, wout = _ptr(out)
        arr = (C.c_void_p * max(k, 1))(*[p for p, _ in ptrs])
        larr = (C.c_size_t * max(k, 1))(*lens)
        xi = np.ascontiguousarray(xi, dtype=np.uint64)
        self.check(self.lib.pc_hip_fr_lincomb(self.h, CURVES[curve], arr, where, larr, k, xi.ctypes.data, pout, wout, n_out))
        return out

    def ligero_commit(self, curve, mat, log_n, col_hash="blake2s", tree_hash="sha256", len_prefix=True,
                      rows=None, in_cols=None, ext_out=None, want_leaves=True):
        """LinearCodePCS::commit steps 1-3 (linear_codes/mod.rs:248-277) in one call: returns
        (nodes (2^h - 1, 32) uint8 with the root at row 0, leaves (2^log_n, 32) uint8 or None)."""
        pin, win = _ptr(mat)
        if rows is None:
            rows, in_cols = mat.shape[0], mat.shape[1]
        hid = {"sha256": 0, "blake2s": 1}
        n = 1 << log_n
        nodes = np.zeros(((1 << max(1, log_n)) - 1, 32), dtype=np.uint8)
        leaves = np.zeros((n, 32), dtype=np.uint8) if want_leaves else None
        pext, wext = _ptr(ext_out) if ext_out is not None else (None, PC_MEM_HOST)
        self.check(self.lib.pc_hip_ligero_commit(self.h, CURVES[curve], pin, win, rows, in_cols, log_n, hid[col_hash],
                                                 hid[tree_hash], 1 if len_prefix else 0, pext, wext,
                                                 leaves.ctypes.data if want_leaves else None, nodes.ctypes.data))
        return nodes, leaves

    def last_ligero_phases_ms(self):
        out = (C.c_float * 4)()
        self.check(self.lib.pc_hip_last_ligero_phases_ms(self.h, out))
        return list(out)

    def last_ntt_phases_ms(self):
        out = (C.c_float * 2)()
        self.check(self.lib.pc_hip_last_ntt_phases_ms(self.h, out))
        return list(out)

    # raw device buffers of the library (pc_hip_malloc / pc_hip_free / pc_hip_memcpy_*): what a shim caches a polynomial in
    def malloc(self, nbytes):
        p = C.c_void_p()
        self.check(self.lib.pc_hip_malloc(self.h, nbytes, C.byref(p)))
        return p.value

    def free_dev(self, ptr):
        self.check(self.lib.pc_hip_free(self.h, C.c_void_p(ptr)))

    def memcpy_h2d(self, dst_dev, src_host):
        src = np.ascontiguousarray(src_host)
        self.check(self.lib.pc_hip_memcpy_h2d(self.h, C.c_void_p(dst_dev), C.c_void_p(src.ctypes.data), src.nbytes))

    def witness_poly(self, curve, coeffs, z, out=None, n=None):
        """q = p / (x - z); coeffs n x 4 uint64 (Montgomery), z 4 x uint64 host array."""
        pin, win = _ptr(coeffs)
        if n is None:
            n = coeffs.shape[0]
        if out is None:
            assert win == PC_MEM_HOST
            out = np.zeros((max(n - 1, 1), 4), dtype=np.uint64)
        pout, wout = _ptr(out)
        z = np.ascontiguousarray(z, dtype=np.uint64)
        self.check(self.lib.pc_hip_witness_poly(self.h, CURVES[curve], pin, win, n, C.c_void_p(z.ctypes.data), pout, wout))
        return out[: max(n - 1, 0)] if isinstance(out, np.ndarray) else out

    def poly_eval(self, curve, coeffs, z, n=None):
        """p(z) of n coefficients (host array or device pointer); returns the Montgomery value, (4,) uint64."""
        pin, win = _ptr(coeffs)
        if n is None:
            n = coeffs.shape[0]
        z = np.ascontiguousarray(z, dtype=np.uint64)
        out = np.zeros(4, dtype=np.uint64)
        self.check(self.lib.pc_hip_poly_eval(self.h, CURVES[curve], pin, win, n, z.ctypes.data, out.ctypes.data))
        return out

    def div_scan(self, curve, coeffs, z, carry_in=None, out=None, n=None):
        """acc = carry_in; for i = n-1..0: acc = coeffs[i] + z*acc; out[i] = acc  (n outputs)."""
        pin, win = _ptr(coeffs)
        if n is None:
            n = coeffs.shape[0]
        if out is None:
            assert win == PC_MEM_HOST
            out = np.zeros((n, 4), dtype=np.uint64)
        pout, wout = _ptr(out)
        z = np.ascontiguousarray(z, dtype=np.uint64)
        cin = None
        if carry_in is not None:
            carry_in = np.ascontiguousarray(carry_in, dtype=np.uint64)
            cin = C.c_void_p(carry_in.ctypes.data)
        self.check(self.lib.pc_hip_poly_div_scan(self.h, CURVES[curve], pin, win, n, C.c_void_p(z.ctypes.data), cin,
                                                 pout, wout))
        return out

    # ---- streaming_kzg: the folding tree and the division by a vanishing polynomial ------------------
    def fold_tree(self, curve, coeffs, challenges, out_dev, out_capacity, n=None):
        """pc_hip_fold_tree: every level f_1 .. f_depth of the folding tree of `coeffs` ((n, 4) uint64 host array or a device pointer
        with n) into the device buffer out_dev; challenges: (depth, 4).  Returns the element offsets of the levels."""
        pin, win = _ptr(coeffs)
        if n is None:
            n = coeffs.shape[0]
        ch = np.ascontiguousarray(challenges, dtype=np.uint64)
        depth = ch.shape[0]
        offs = (C.c_size_t * max(depth, 1))()
        self.check(self.lib.pc_hip_fold_tree(self.h, CURVES[curve], pin, win, n, C.c_void_p(ch.ctypes.data), depth, C.c_void_p(out_dev), out_capacity, offs))
        return list(offs)[:depth]

    def poly_div_multi(self, curve, coeffs, points, n=None, want_quotient=True):
        """pc_hip_poly_div_multi: (q, r) = (p div Z, p mod Z), Z = prod (x - points[j]); r: (k, 4), highest degree first; q: (max(n - k,
        0), 4) on the host, or None."""
        pin, win = _ptr(coeffs)
        if n is None:
            n = coeffs.shape[0]
        z = np.ascontiguousarray(points, dtype=np.uint64)
        k = z.shape[0]
        q = np.zeros((max(n - k, 0), 4), dtype=np.uint64) if want_quotient else None
        r = np.zeros((k, 4), dtype=np.uint64)
        self.check(self.lib.pc_hip_poly_div_multi(self.h, CURVES[curve], pin, win, n, C.c_void_p(z.ctypes.data), k,
                                                  C.c_void_p(q.ctypes.data) if want_quotient and q.size else None, PC_MEM_HOST, C.c_void_p(r.ctypes.data)))
        return q, r

    def last_skzg_launches(self):
        """kernel launches of the last streaming_kzg call: (folding tree, divisions + combination)"""
        out = (C.c_uint * 2)()
        self.check(self.lib.pc_hip_last_skzg_launches(self.h, out))
        return int(out[0]), int(out[1])

    # ---- MarlinPST13: the dense lexicographic layout (include/pc_hip.h) -------------------------------
    def pst13_monomial_evals(self, curve, num_vars, degree, betas, out_dev):
        """pc_hip_pst13_monomial_evals: out_dev[rank(e)] = prod_j betas[j]^e_j for all M ranks; betas: (num_vars, 4) uint64"""
        b = np.ascontiguousarray(betas, dtype=np.uint64)
        assert b.shape == (num_vars, 4)
        self.check(self.lib.pc_hip_pst13_monomial_evals(self.h, CURVES[curve], num_vars, degree, C.c_void_p(b.ctypes.data), C.c_void_p(out_dev)))

    def pst13_scatter(self, curve, num_vars, degree, exps, coeffs, out_dev, n_terms=None):
        """pc_hip_pst13_scatter: the terms (exps (T, num_vars) uint8, coeffs (T, 4) uint64; or device pointers with n_terms) into the
        dense device vector out_dev of M elements"""
        pe, pc_, where, count, keep = _pst13_terms(num_vars, exps, coeffs, n_terms)
        self.check(self.lib.pc_hip_pst13_scatter(self.h, CURVES[curve], num_vars, degree, pe, pc_, where, count, C.c_void_p(out_dev)))
        del keep

    def pst13_divide(self, curve, num_vars, degree, poly, point, quotients_dev, capacity):
        """pc_hip_pst13_divide: the num_vars quotients of divide_at_point packed into quotients_dev.  poly: (M, 4) uint64 host array or
        a device pointer; point: (num_vars, 4).  Returns (element offsets, p(z) as (4,) uint64)."""
        pp, where = _ptr(poly)
        z = np.ascontiguousarray(point, dtype=np.uint64)
        assert z.shape == (num_vars, 4)
        offs = (C.c_size_t * num_vars)()
        value = np.zeros(4, dtype=np.uint64)
        self.check(self.lib.pc_hip_pst13_divide(self.h, CURVES[curve], num_vars, degree, pp, where, C.c_void_p(z.ctypes.data), C.c_void_p(quotients_dev),
                                                capacity, offs, C.c_void_p(value.ctypes.data)))
        return list(offs), value

    def last_pst13_shape(self):
        """the last pst13_open: (univariate route?, [pairs of MSM 0, 1, ..]) (pc_hip_last_pst13_shape)"""
        out = (C.c_uint32 * (2 + PST13_MAX_VARS))()
        self.check(self.lib.pc_hip_last_pst13_shape(self.h, out))
        return bool(out[1]), [int(v) for v in out[2:2 + int(out[0])]]

    # ---- IPA round primitives (device-resident vectors; `dev` = raw device pointer) --------------
    def fr_fold(self, curve, lo_dev, hi_dev, n_half, s):
        s = np.ascontiguousarray(s, dtype=np.uint64)
        self.check(self.lib.pc_hip_fr_fold(self.h, CURVES[curve], lo_dev, hi_dev, n_half, C.c_void_p(s.ctypes.data)))

    def fr_dot(self, curve, a_dev, b_dev, n):
        out = np.zeros(4, dtype=np.uint64)
        self.check(self.lib.pc_hip_fr_dot(self.h, CURVES[curve], a_dev, b_dev, n, C.c_void_p(out.ctypes.data)))
        return out

    def ipa_fold_dots(self, curve, coeffs_dev, z_dev, m, u=None, u_inv=None):
        """pc_hip_ipa_fold_dots: optional fold at size 2m by (u, u^-1), then the round's two inner products at size m -> (2, 4) uint64."""
        out = np.zeros((2, 4), dtype=np.uint64)
        pu = pi = None
        if u is not None:
            u = np.ascontiguousarray(u, dtype=np.uint64); u_inv = np.ascontiguousarray(u_inv, dtype=np.uint64)
            pu, pi = C.c_void_p(u.ctypes.data), C.c_void_p(u_inv.ctypes.data)
        self.check(self.lib.pc_hip_ipa_fold_dots(self.h, CURVES[curve], coeffs_dev, z_dev, m, pu, pi, C.c_void_p(out.ctypes.data)))
        return out

    def fr_powers(self, curve, z, n, out_dev):
        z = np.ascontiguousarray(z, dtype=np.uint64)
        self.check(self.lib.pc_hip_fr_powers(self.h, CURVES[curve], C.c_void_p(z.ctypes.data), n, out_dev))

    def ipa_key_scalars(self, curve, coeffs_dev, m, s_dev, n0, fold_u=None, fold_m=0, out_l_dev=None, out_r_dev=None):
        """pc_hip_ipa_key_scalars: fold the key factors s by fold_u (optional), build the round's MSM scalars (optional)."""
        fu = None
        if fold_u is not None:
            fold_u = np.ascontiguousarray(fold_u, dtype=np.uint64)
            fu = C.c_void_p(fold_u.ctypes.data)
        self.check(self.lib.pc_hip_ipa_key_scalars(self.h, CURVES[curve], coeffs_dev, m, s_dev, n0, fu, fold_m, out_l_dev, out_r_dev))

    def fixed_base_batch_mul(self, curve, g_xy, scalars_dev, n, out_dev):
        """out[i] = scalars[i] * g (device buffers): the SRS generation of KZG10::setup."""
        g_xy = np.ascontiguousarray(g_xy, dtype=np.uint64)
        self.check(self.lib.pc_hip_fixed_base_batch_mul(self.h, CURVES[curve], C.c_void_p(g_xy.ctypes.data), scalars_dev, n, out_dev))

    def upload_srs(self, curve, bases, n=None, stride_bytes=0):
        return Srs(self, curve, bases, n, stride_bytes)

    def upload_g2_srs(self, curve, bases, n=None, stride_bytes=0):
        return G2Srs(self, curve, bases, n, stride_bytes)

    def upload_te_srs(self, curve, bases, n=None, stride_bytes=0):
        """A resident key of twisted Edwards points (pc_hip_te_srs_upload); curve: a name of TE_CURVES, bases: n x 64 bytes x || y."""
        return TeSrs(self, curve, bases, n, stride_bytes)

    def te_sample_generators(self, curve, protocol_name, first_index, count, want_digests=False):
        """InnerProductArgPC::sample_generators on the device (pc_hip_te_sample_generators): generators [first_index, first_index + count)
        of the byte string protocol_name (at most 48 bytes) as a new resident TeSrs; with want_digests also the uint32 array of the
        digests every index consumed (1: the first one was accepted)."""
        name = bytes(protocol_name)
        digests = np.zeros(max(count, 1), dtype=np.uint32) if want_digests else None
        h = C.c_void_p()
        self.check(self.lib.pc_hip_te_sample_generators(self.h, TE_CURVES[curve], name, len(name), first_index, count,
                                                        digests.ctypes.data_as(C.POINTER(C.c_uint32)) if want_digests else None, C.byref(h)))
        key = TeSrs._adopt(self, curve, h, count)
        return (key, digests[:count]) if want_digests else key

    def sample_generators(self, curve, protocol_name, first_index, count, want_digests=False):
        """sample_generators over a short Weierstrass curve on the device (pc_hip_sample_generators; ipa_pc/mod.rs:302-325,
        hyrax/mod.rs:119-168): generators [first_index, first_index + count) of the byte string protocol_name (at most 48 bytes) as a
        new resident Srs; with want_digests also the uint32 array of the digests every index consumed (1: the first one was accepted)."""
        name = bytes(protocol_name)
        digests = np.zeros(max(count, 1), dtype=np.uint32) if want_digests else None
        h = C.c_void_p()
        self.check(self.lib.pc_hip_sample_generators(self.h, CURVES[curve], name, len(name), first_index, count,
                                                     digests.ctypes.data_as(C.POINTER(C.c_uint32)) if want_digests else None, C.byref(h)))
        key = Srs._adopt(self, curve, h, count)
        return (key, digests[:count]) if want_digests else key

    def te_fr_powers(self, curve, z_mont, n, out_dev):
        """out_dev[i] = z^i, i < n, over the scalar field of a twisted Edwards curve (pc_hip_te_fr_powers); z_mont: 32 bytes, host."""
        z = np.ascontiguousarray(z_mont)
        self.check(self.lib.pc_hip_te_fr_powers(self.h, TE_CURVES[curve], C.c_void_p(z.ctypes.data), n, _ptr(out_dev)[0]))

    def te_fr_dot(self, curve, a_dev, b_dev, n):
        """<a, b> over the scalar field of a twisted Edwards curve (pc_hip_te_fr_dot): two device vectors of n Montgomery Fr -> 32 bytes."""
        out = np.zeros(32, dtype=np.uint8)
        self.check(self.lib.pc_hip_te_fr_dot(self.h, TE_CURVES[curve], _ptr(a_dev)[0], _ptr(b_dev)[0], n, C.c_void_p(out.ctypes.data)))
        return out

    def te_fr_lincomb(self, curve, polys, xi, n_out=None, out=None, lens=None):
        """sum_j xi[j] * polys[j] over the scalar field of a twisted Edwards curve (pc_hip_te_fr_lincomb; Hyrax's row_mul).
        polys: list of (len_j, 32) uint8 host arrays, or device pointers with `lens`; xi: (k, 32) uint8 Montgomery Fr on the host.
        Returns `out` (a device pointer / tensor if given, else a new (n_out, 32) uint8 host array)."""
        k = len(polys)
        ptrs = [_ptr(p) for p in polys]
        where = ptrs[0][1] if k else PC_MEM_HOST
        assert all(w == where for _, w in ptrs)
        if lens is None:
            lens = [p.shape[0] for p in polys]
        if n_out is None:
            n_out = max(lens) if k else 0
        if out is None:
            out = np.zeros((n_out, 32), dtype=np.uint8)
        pout, wout = _ptr(out)
        arr = (C.c_void_p * max(k, 1))(*[p for p, _ in ptrs])
        larr = (C.c_size_t * max(k, 1))(*lens)
        xi = np.ascontiguousarray(xi)
        self.check(self.lib.pc_hip_te_fr_lincomb(self.h, TE_CURVES[curve], arr, where, larr, k, C.c_void_p(xi.ctypes.data), pout, wout, n_out))
        return out

    def te_ipa_fold_dots(self, curve, coeffs_dev, z_dev, m, u=None, u_inv=None):
        """pc_hip_te_ipa_fold_dots: optional fold at size 2m by (u, u^-1), then the round's two inner products at size m -> (2, 32) uint8."""
        out = np.zeros((2, 32), dtype=np.uint8)
        pu = pi = None
        if u is not None:
            u, u_inv = np.ascontiguousarray(u), np.ascontiguousarray(u_inv)
            pu, pi = C.c_void_p(u.ctypes.data), C.c_void_p(u_inv.ctypes.data)
        self.check(self.lib.pc_hip_te_ipa_fold_dots(self.h, TE_CURVES[curve], _ptr(coeffs_dev)[0], _ptr(z_dev)[0], m, pu, pi, C.c_void_p(out.ctypes.data)))
        return out

    def te_ipa_key_scalars(self, curve, coeffs_dev, m, s_dev, n0, fold_u=None, fold_m=0, out_l_dev=None, out_r_dev=None):
        """pc_hip_te_ipa_key_scalars: fold the key factors s by fold_u (optional), build the round's MSM scalars (optional)."""
        fu = None
        if fold_u is not None:
            fold_u = np.ascontiguousarray(fold_u)
            fu = C.c_void_p(fold_u.ctypes.data)
        opt = lambda x: None if x is None else _ptr(x)[0]
        self.check(self.lib.pc_hip_te_ipa_key_scalars(self.h, TE_CURVES[curve], opt(coeffs_dev), m, _ptr(s_dev)[0], n0, fu, fold_m, opt(out_l_dev), opt(out_r_dev)))

    def ml_fold(self, curve, r_in_dev, n_half, z, r_out_dev, q_dev):
        """One halving round of MultilinearPC::open on device vectors (pc_hip_ml_fold); z: one Montgomery Fr (host)."""
        z = np.ascontiguousarray(z)
        self.check(self.lib.pc_hip_ml_fold(self.h, CURVES[curve], r_in_dev, n_half, C.c_void_p(z.ctypes.data), r_out_dev, q_dev))

    def ml_eq_evals(self, curve, t, nv, out_dev):
        """out_dev[x] = prod_j e(t_j, bit_j(x)), 2^nv Montgomery Fr on the device (pc_hip_ml_eq_evals); t: nv Montgomery Fr (host)."""
        t = np.ascontiguousarray(t)
        self.check(self.lib.pc_hip_ml_eq_evals(self.h, CURVES[curve], C.c_void_p(t.ctypes.data), nv, out_dev))

    def g2_fixed_base_batch_mul(self, curve, h_point, scalars_dev, n, out_dev):
        """out[i] = scalars[i] * h for one G2 point (device buffers): `h.batch_mul` of MultilinearPC::setup."""
        h_point = np.ascontiguousarray(h_point)
        self.check(self.lib.pc_hip_g2_fixed_base_batch_mul(self.h, CURVES[curve], C.c_void_p(h_point.ctypes.data), scalars_dev, n, out_dev))

    def ml_setup(self, curve, nv, g, h, t):
        """MultilinearPC::setup on the device (pc_hip_ml_setup) from g (96 bytes), h (192 bytes) and the trapdoor t (nv Montgomery Fr).
        Returns (powers_of_g: Srs of 2^(nv+1) - 2 points, powers_of_h: G2Srs of 2^(nv+1) - 1 points with h last, g_mask: nv x 96 bytes);
        level i of either key starts at ml_level_offset(nv, i)."""
        g, h, t = np.ascontiguousarray(g), np.ascontiguousarray(h), np.ascontiguousarray(t)
        mask = np.zeros((nv, 2 * FQ_BYTES[curve]), dtype=np.uint8)
        hg, hh = C.c_void_p(), C.c_void_p()
        self.check(self.lib.pc_hip_ml_setup(self.h, CURVES[curve], nv, C.c_void_p(g.ctypes.data), C.c_void_p(h.ctypes.data), C.c_void_p(t.ctypes.data),
                                            C.byref(hg), C.byref(hh), C.c_void_p(mask.ctypes.data)))
        return Srs._adopt(self, curve, hg, (2 << nv) - 2), G2Srs._adopt(self, curve, hh, (2 << nv) - 1), mask

    def ml_trim(self, powers_of_g, powers_of_h, nv, supported):
        """MultilinearPC::trim from resident parameters (pc_hip_ml_trim): (Srs of level nv - supported, 2^supported points; the pair-sum
        G2Srs of 2^supported - 1 points that ml_open takes)."""
        hg, hh = C.c_void_p(), C.c_void_p()
        self.check(self.lib.pc_hip_ml_trim(self.h, powers_of_g.h, powers_of_h.h, nv, supported, C.byref(hg), C.byref(hh)))
        return Srs._adopt(self, powers_of_g.curve, hg, 1 << supported), G2Srs._adopt(self, powers_of_h.curve, hh, (1 << supported) - 1)

    def brakedown_code(self, curve, msg_len, codeword_len, dims=(), ind_ptr=(), col_ind=(), val=None):
        """Resident Brakedown code (pc_hip_brakedown_code_create) from the caller's sampled matrices."""
        return BrakedownCode(self, curve, msg_len, codeword_len, dims, ind_ptr, col_ind, val)

    def last_brakedown_phases_ms(self):
        out = (C.c_float * 4)()
        self.check(self.lib.pc_hip_last_brakedown_phases_ms(self.h, out))
        return list(out)

    def bytes_resident(self):
        """pc_hip_ctx_bytes_resident: device bytes by kind."""
        out = (C.c_size_t * 6)()
        self.check(self.lib.pc_hip_ctx_bytes_resident(self.h, out))
        return dict(zip(("device_total", "keys", "window_tables", "fold_tables", "scratch", "n_keys"), [int(x) for x in out]))

    def trim(self):
        self.check(self.lib.pc_hip_ctx_trim(self.h))

    def load_serialized_srs(self, curve, data, compressed, max_points=0, validate=None):
        """Resident SRS from the ark-serialize bytes of a Vec<G1Affine> (the head of kzg10::UniversalParams):
        returns (Srs, bytes_consumed).  validate: None is pc_hip_srs_load_serialized (Validate::No plus the curve equation); an integer
        of CHECK_ON_CURVE | CHECK_SUBGROUP goes to pc_hip_srs_load_serialized_ex, and True is both bits: Validate::Yes."""
        h, npts, used = C.c_void_p(), C.c_size_t(), C.c_size_t()
        buf = (C.c_char * len(data)).from_buffer_copy(data)
        if validate is None:
            self.check(self.lib.pc_hip_srs_load_serialized(self.h, CURVES[curve], buf, len(data), 1 if compressed else 0, max_points,
                                                           C.byref(h), C.byref(npts), C.byref(used)))
        else:
            what = (CHECK_ON_CURVE | CHECK_SUBGROUP) if validate is True else int(validate)
            self.check(self.lib.pc_hip_srs_load_serialized_ex(self.h, CURVES[curve], buf, len(data), 1 if compressed else 0, max_points,
                                                              what, C.byref(h), C.byref(npts), C.byref(used)))
        srs = Srs.__new__(Srs)
        srs.ctx, srs.curve, srs.h, srs.n = self, curve, h, npts.value
        return srs, used.value


CHECK_ON_CURVE, CHECK_SUBGROUP = 1, 2      # PC_HIP_CHECK_ON_CURVE, PC_HIP_CHECK_SUBGROUP


def _key_check(ctx, fn, handle, n, offset, count, on_curve, subgroup, want_flags):
    """pc_hip_srs_check / pc_hip_g2_srs_check -> (bad, first_bad or None[, flags])"""
    count = n - offset if count is None else count
    what = (CHECK_ON_CURVE if on_curve else 0) | (CHECK_SUBGROUP if subgroup else 0)
    bad, first = C.c_size_t(), C.c_size_t()
    flags = np.zeros(count, dtype=np.uint8) if want_flags else None
    ctx.check(fn(ctx.h, handle, offset, count, what, C.byref(bad), C.byref(first), C.c_void_p(flags.ctypes.data) if want_flags else None))
    out = (bad.value, first.value if bad.value else None)
    return out + (flags,) if want_flags else out


class BrakedownCode:
    """Resident sparse matrices of one Brakedown code (pc_lincode).  dims: (n, m, d) per matrix, the A matrices first, then the B
    matrices; ind_ptr: m + 1 numbers per matrix, each matrix counting from 0; col_ind / val ((nnz, 4) uint64, Montgomery): the
    matrices' entries back to back.  The library copies the arrays: nothing of them is referenced after construction."""

    def __init__(self, ctx, curve, msg_len, codeword_len, dims=(), ind_ptr=(), col_ind=(), val=None):
        self.ctx, self.curve, self.msg_len = ctx, curve, msg_len
        dims = np.ascontiguousarray(dims, dtype=np.uintp).reshape(-1)
        ind_ptr = np.ascontiguousarray(ind_ptr, dtype=np.uintp).reshape(-1)
        col_ind = np.ascontiguousarray(col_ind, dtype=np.uint32).reshape(-1)
        val = np.zeros((0, 4), dtype=np.uint64) if val is None else np.ascontiguousarray(val, dtype=np.uint64).reshape(-1, 4)
        assert len(dims) % 6 == 0 and len(val) == len(col_ind)
        h = C.c_void_p()
        ctx.check(ctx.lib.pc_hip_brakedown_code_create(ctx.h, CURVES[curve], msg_len, codeword_len, len(dims) // 6, dims.ctypes.data, ind_ptr.ctypes.data,
                                                       col_ind.ctypes.data, val.ctypes.data, len(col_ind), C.byref(h)))
        self.h = h
        self.codeword_len = int(ctx.lib.pc_hip_brakedown_codeword_len(h))

    def free(self):
        if self.h:
            self.ctx.lib.pc_hip_brakedown_code_free(self.h)
            self.h = None

    def encode(self, msgs, rows=None, out=None):
        """rows x msg_len (Montgomery) -> rows x codeword_len, row-major: numpy in -> numpy out; torch cuda tensors / device pointers
        (with rows, out) stay on the device."""
        pin, win = _ptr(msgs)
        if rows is None:
            rows = msgs.shape[0]
        if out is None:
            assert win == PC_MEM_HOST
            out = np.zeros((rows, self.codeword_len, 4), dtype=np.uint64)
        pout, wout = _ptr(out)
        self.ctx.check(self.ctx.lib.pc_hip_brakedown_encode(self.ctx.h, self.h, pin, win, rows, pout, wout))
        return out

    def commit(self, mat, rows=None, col_hash="blake2s", tree_hash="sha256", len_prefix=True, ext_out=None, want_leaves=True):
        """LinearCodePCS::commit steps 1-3 (pc_hip_brakedown_commit): (nodes (2^h - 1, 32) uint8, root first; leaves (codeword_len, 32) or None)."""
        pin, win = _ptr(mat)
        if rows is None:
            rows = mat.shape[0]
        hid = {"sha256": 0, "blake2s": 1}
        n = self.codeword_len
        nodes = np.zeros(((1 << max(1, (n - 1).bit_length())) - 1, 32), dtype=np.uint8)
        leaves = np.zeros((n, 32), dtype=np.uint8) if want_leaves else None
        pext, wext = _ptr(ext_out) if ext_out is not None else (None, PC_MEM_HOST)
        self.ctx.check(self.ctx.lib.pc_hip_brakedown_commit(self.ctx.h, self.h, pin, win, rows, hid[col_hash], hid[tree_hash], 1 if len_prefix else 0,
                                                            pext, wext, leaves.ctypes.data if want_leaves else None, nodes.ctypes.data))
        return nodes, leaves


class Srs:
    """Resident bases (pc_srs): powers_of_g of a KZG committer key, or an IPA comm_key."""

    def __init__(self, ctx, curve, bases, n=None, stride_bytes=0):
        self.ctx, self.curve = ctx, curve
        p, where = _ptr(bases)
        if n is None:
            n = bases.shape[0]
        h = C.c_void_p()
        ctx.check(ctx.lib.pc_hip_srs_upload(ctx.h, CURVES[curve], p, n, stride_bytes, where, C.byref(h)))
        self.h, self.n = h, n

    def precompute(self, window_bits=0, min_pairs=0, glv=None):
        """Build the window table of this SRS in HBM (pc_hip_srs_precompute).  glv=True: the half-size table over the GLV halves of
        the scalars (pc_hip_srs_precompute_ex, PC_HIP_TABLE_GLV); False: the full table; None: the library's policy."""
        if glv is None:
            self.ctx.check(self.ctx.lib.pc_hip_srs_precompute(self.ctx.h, self.h, window_bits, min_pairs))
        else:
            self.ctx.check(self.ctx.lib.pc_hip_srs_precompute_ex(self.ctx.h, self.h, window_bits, min_pairs, 1 if glv else 0))
        return self

    @classmethod
    def _adopt(cls, ctx, curve, handle, n):
        """wrap a key the library made (pc_hip_ml_setup, pc_hip_ml_trim)"""
        out = cls.__new__(cls)
        out.ctx, out.curve, out.h, out.n = ctx, curve, handle, n
        return out

    def free(self):
        if self.h:
            self.ctx.lib.pc_hip_srs_free(self.h)
            self.h = None

    def msm(self, scalars, n=None, base_offset=0, montgomery=False):
        """sum scalars[i] * bases[base_offset + i]; returns (xy uint64 array, is_infinity)."""
        p, where = _ptr(scalars)
        if n is None:
            n = scalars.shape[0]
        out = np.zeros(2 * FQ_BYTES[self.curve] // 8, dtype=np.uint64)
        inf = C.c_int(0)
        self.ctx.check(self.ctx.lib.pc_hip_msm(self.ctx.h, self.h, base_offset, p,
                                               PC_SCALARS_MONTGOMERY if montgomery else PC_SCALARS_CANONICAL,
                                               where, n, C.c_void_p(out.ctypes.data), C.byref(inf)))
        return out, bool(inf.value)

    def kzg_open(self, coeffs, z, n=None, base_offset=0):
        """KZG10::open without hiding as one call (pc_hip_kzg_open): W = MSM(bases[base_offset ..], p / (x - z)); coeffs: (n, 4)
        uint64 host array (Montgomery) or a device pointer with n.  Returns (xy uint64 array, is_infinity)."""
        p, where = _ptr(coeffs)
        if n is None:
            n = coeffs.shape[0]
        z = np.ascontiguousarray(z, dtype=np.uint64)
        out = np.zeros(2 * FQ_BYTES[self.curve] // 8, dtype=np.uint64)
        inf = C.c_int(0)
        self.ctx.check(self.ctx.lib.pc_hip_kzg_open(self.ctx.h, self.h, base_offset, p, where, n, C.c_void_p(z.ctypes.data),
                                                    C.c_void_p(out.ctypes.data), C.byref(inf)))
        return out, bool(inf.value)

    def _point_out(self):
        return np.zeros(2 * FQ_BYTES[self.curve] // 8, dtype=np.uint64), C.c_int(0)

    def kzg_open_multi(self, coeffs, points, n=None, base_offset=0):
        """open_multi_points of streaming_kzg as one call (pc_hip_kzg_open_multi): one proof for p at all `points` ((k, 4) uint64).
        Returns (xy, is_infinity, remainder (k, 4) highest degree first)."""
        p, where = _ptr(coeffs)
        if n is None:
            n = coeffs.shape[0]
        z = np.ascontiguousarray(points, dtype=np.uint64)
        r = np.zeros((z.shape[0], 4), dtype=np.uint64)
        out, inf = self._point_out()
        self.ctx.check(self.ctx.lib.pc_hip_kzg_open_multi(self.ctx.h, self.h, base_offset, p, where, n, C.c_void_p(z.ctypes.data), z.shape[0],
                                                          C.c_void_p(r.ctypes.data), C.c_void_p(out.ctypes.data), C.byref(inf)))
        return out, bool(inf.value), r

    def kzg_batch_open_multi(self, polys, points, eta, lens=None, base_offset=0):
        """batch_open_multi_points (pc_hip_kzg_batch_open_multi): the proof of sum_j eta^j polys[j] at all `points`.  polys: host arrays,
        or device pointers with `lens`.  Returns (xy, is_infinity)."""
        ptrs = [_ptr(p) for p in polys]
        where = ptrs[0][1]
        assert all(w == where for _, w in ptrs)
        if lens is None:
            lens = [p.shape[0] for p in polys]
        arr = (C.c_void_p * len(polys))(*[p for p, _ in ptrs])
        larr = (C.c_size_t * len(polys))(*lens)
        z = np.ascontiguousarray(points, dtype=np.uint64)
        eta = np.ascontiguousarray(eta, dtype=np.uint64)
        out, inf = self._point_out()
        self.ctx.check(self.ctx.lib.pc_hip_kzg_batch_open_multi(self.ctx.h, self.h, base_offset, arr, where, larr, len(polys), C.c_void_p(z.ctypes.data),
                                                                z.shape[0], C.c_void_p(eta.ctypes.data), C.c_void_p(out.ctypes.data), C.byref(inf)))
        return out, bool(inf.value)

    def kzg_commit_folding(self, coeffs, challenges, n=None, base_offset=0):
        """commit_folding (pc_hip_kzg_commit_folding): the commitments of the levels f_1 .. f_depth of the folding tree.
        Returns ((depth, 2*Fq limbs) points, (depth,) infinity flags)."""
        p, where = _ptr(coeffs)
        if n is None:
            n = coeffs.shape[0]
        ch = np.ascontiguousarray(challenges, dtype=np.uint64)
        depth = ch.shape[0]
        out = np.zeros((depth, 2 * FQ_BYTES[self.curve] // 8), dtype=np.uint64)
        inf = (C.c_int * max(depth, 1))()
        self.ctx.check(self.ctx.lib.pc_hip_kzg_commit_folding(self.ctx.h, self.h, base_offset, p, where, n, C.c_void_p(ch.ctypes.data), depth,
                                                              C.c_void_p(out.ctypes.data), inf))
        return out, np.array(list(inf)[:depth], dtype=bool)

    def kzg_open_folding(self, coeffs, challenges, points, etas, n=None, base_offset=0):
        """open_folding (pc_hip_kzg_open_folding): every level's remainder modulo Z and the one proof over the eta-combined quotients.
        Returns (remainders (depth, k, 4) highest degree first, xy, is_infinity)."""
        p, where = _ptr(coeffs)
        if n is None:
            n = coeffs.shape[0]
        ch = np.ascontiguousarray(challenges, dtype=np.uint64)
        z = np.ascontiguousarray(points, dtype=np.uint64)
        et = np.ascontiguousarray(etas, dtype=np.uint64)
        depth, k = ch.shape[0], z.shape[0]
        assert et.shape[0] == depth
        rem = np.zeros((depth, k, 4), dtype=np.uint64)
        out, inf = self._point_out()
        self.ctx.check(self.ctx.lib.pc_hip_kzg_open_folding(self.ctx.h, self.h, base_offset, p, where, n, C.c_void_p(ch.ctypes.data), depth,
                                                            C.c_void_p(z.ctypes.data), k, C.c_void_p(et.ctypes.data), C.c_void_p(rem.ctypes.data),
                                                            C.c_void_p(out.ctypes.data), C.byref(inf)))
        return rem, out, bool(inf.value)

    def pst13_commit(self, num_vars, degree, dense=None, exps=None, coeffs=None, n_terms=None, base_offset=0):
        """MarlinPST13::commit without hiding (pc_hip_pst13_commit) of a dense vector ((M, 4) uint64 host array or a device pointer) or
        of terms (as Context.pst13_scatter).  Returns (xy, is_infinity)."""
        pd, wd = _ptr(dense) if dense is not None else (None, PC_MEM_HOST)
        pe, pc_, wt, count, keep = _pst13_terms(num_vars, exps, coeffs, n_terms)
        out, inf = self._point_out()
        self.ctx.check(self.ctx.lib.pc_hip_pst13_commit(self.ctx.h, self.h, base_offset, num_vars, degree, pd, wd, pe, pc_, wt, count,
                                                        C.c_void_p(out.ctypes.data), C.byref(inf)))
        del keep
        return out, bool(inf.value)

    def pst13_open(self, num_vars, degree, point, dense=None, exps=None, coeffs=None, n_terms=None, base_offset=0):
        """MarlinPST13::open without hiding (pc_hip_pst13_open).  Returns ((num_vars, 2*Fq limbs) points w_i, (num_vars,) infinity flags,
        p(point) as (4,) uint64)."""
        pd, wd = _ptr(dense) if dense is not None else (None, PC_MEM_HOST)
        pe, pc_, wt, count, keep = _pst13_terms(num_vars, exps, coeffs, n_terms)
        z = np.ascontiguousarray(point, dtype=np.uint64)
        assert z.shape == (num_vars, 4)
        out = np.zeros((num_vars, 2 * FQ_BYTES[self.curve] // 8), dtype=np.uint64)
        inf = (C.c_int * num_vars)()
        value = np.zeros(4, dtype=np.uint64)
        self.ctx.check(self.ctx.lib.pc_hip_pst13_open(self.ctx.h, self.h, base_offset, num_vars, degree, pd, wd, pe, pc_, wt, count,
                                                      C.c_void_p(z.ctypes.data), C.c_void_p(out.ctypes.data), inf, C.c_void_p(value.ctypes.data)))
        del keep
        return out, np.array(list(inf), dtype=bool), value

    def pst13_trim(self, num_vars, degree, supported_degree, base_offset=0):
        """MarlinPST13::trim's selection (pc_hip_pst13_trim): a new key in the layout (num_vars, supported_degree)"""
        h = C.c_void_p()
        self.ctx.check(self.ctx.lib.pc_hip_pst13_trim(self.ctx.h, self.h, base_offset, num_vars, degree, supported_degree, C.byref(h)))
        return Srs._adopt(self.ctx, self.curve, h, pst13_key_len(num_vars, supported_degree))

    def msm_many(self, scalars, m=None, n_msms=None, base_offset=0, montgomery=False):
        """n_msms MSMs of m pairs over bases[base_offset : base_offset + m] (pc_hip_msm_many; Hyrax's
        one commitment per matrix row).  scalars: (n_msms, m, 4) uint64 host array or a device pointer.
        Returns ((n_msms, 2*Fq limbs) uint64 affine points, (n_msms,) infinity flags)."""
        p, where = _ptr(scalars)
        if m is None:
            n_msms, m = scalars.shape[0], scalars.shape[1]
        out = np.zeros((n_msms, 2 * FQ_BYTES[self.curve] // 8), dtype=np.uint64)
        inf = (C.c_int * max(n_msms, 1))()
        self.ctx.check(self.ctx.lib.pc_hip_msm_many(self.ctx.h, self.h, base_offset, p,
                                                    PC_SCALARS_MONTGOMERY if montgomery else PC_SCALARS_CANONICAL, where, m, n_msms,
                                                    C.c_void_p(out.ctypes.data), inf))
        return out, np.array(list(inf)[:n_msms], dtype=bool)

    def msm_batch(self, scalar_ptrs, lens, base_offsets=None, montgomery=True, host=False):
        """pc_hip_msm_batch: k scalar vectors against this SRS -> (k, 2*Fq) points.  scalar_ptrs: device pointers, or (host=True) host
        numpy arrays / addresses (what MarlinKZG10::commit hands over: the library stages them pass by pass)."""
        k = len(scalar_ptrs)
        if host:
            scalar_ptrs = [p.ctypes.data if isinstance(p, np.ndarray) else p for p in scalar_ptrs]
        ptrs = (C.c_void_p * k)(*scalar_ptrs)
        ns = (C.c_size_t * k)(*lens)
        offs = (C.c_size_t * k)(*base_offsets) if base_offsets is not None else None
        out = np.zeros((k, 2 * FQ_BYTES[self.curve] // 8), dtype=np.uint64)
        infs = (C.c_int * k)()
        self.ctx.check(self.ctx.lib.pc_hip_msm_batch(self.ctx.h, self.h, offs, ptrs, ns, k,
                                                     PC_SCALARS_MONTGOMERY if montgomery else PC_SCALARS_CANONICAL,
                                                     PC_MEM_HOST if host else PC_MEM_DEVICE, C.c_void_p(out.ctypes.data), infs))
        return out

    def ec_fold(self, n_half, u):
        """key[i] = affine(key[i] + u * key[n_half + i]) in place on the resident key."""
        u = np.ascontiguousarray(u, dtype=np.uint64)
        self.ctx.check(self.ctx.lib.pc_hip_ec_fold(self.ctx.h, self.h, n_half, C.c_void_p(u.ctypes.data)))

    def precompute_fold(self, levels=None, naf_width=None):
        """Fold table of this (committer) key: pc_hip_srs_precompute_fold (the library's choice of form), or
        pc_hip_srs_precompute_fold_ex(levels, naf_width) -- levels 1: the upper half (first fold of an opening), 2: the upper three
        quarters (the first two folds in one step, fold2_from); naf_width 2 .. 5; 0 = the library chooses that parameter."""
        if levels is None and naf_width is None:
            self.ctx.check(self.ctx.lib.pc_hip_srs_precompute_fold(self.ctx.h, self.h))
        else:
            self.ctx.check(self.ctx.lib.pc_hip_srs_precompute_fold_ex(self.ctx.h, self.h, levels or 0, naf_width or 0))
        return self

    def fold_table_info(self):
        """(levels, naf_width) of the fold table on this key; (0, 0): none."""
        a, b = C.c_uint(), C.c_uint()
        self.ctx.check(self.ctx.lib.pc_hip_srs_fold_table_info(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def ipa_open_rounds(self, coeffs_dev, n, point_mont, h_prime_xy, next_challenge, fixed_key_below=0, want_times=False):
        """The whole halving loop of InnerProductArgPC::open on this resident committer key (pc_hip_ipa_open_rounds).
        next_challenge(l_xy, r_xy) -> u as 4 Montgomery uint64 limbs.  Returns (l_vec, r_vec, final_key, c[, round_ms, fold_ms])."""
        lg = n.bit_length() - 1
        w = 2 * FQ_BYTES[self.curve] // 8
        l = np.zeros((max(lg, 1), w), dtype=np.uint64)
        r = np.zeros((max(lg, 1), w), dtype=np.uint64)
        fk, c = np.zeros(w, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
        err = []

        def cb(_user, lp, rp, up):
            try:
                lxy = np.frombuffer((C.c_uint64 * w).from_address(lp), dtype=np.uint64).copy()
                rxy = np.frombuffer((C.c_uint64 * w).from_address(rp), dtype=np.uint64).copy()
                u = np.ascontiguousarray(next_challenge(lxy, rxy), dtype=np.uint64)
                C.memmove(up, u.ctypes.data, 32)
            except BaseException as e:      # an exception must not cross the C frames: finish the loop on a dummy challenge, raise afterwards
                err.append(e)
                C.memset(up, 0, 32); C.memset(up, 1, 1)
        fn = IPA_CHALLENGE_FN(cb)
        point = np.ascontiguousarray(point_mont, dtype=np.uint64)
        hp = np.ascontiguousarray(h_prime_xy, dtype=np.uint64)
        rms = (C.c_float * max(lg, 1))()
        fms = (C.c_float * max(lg, 1))()
        p, _ = _ptr(coeffs_dev)
        rc = self.ctx.lib.pc_hip_ipa_open_rounds(self.ctx.h, self.h, p, n, C.c_void_p(point.ctypes.data), C.c_void_p(hp.ctypes.data), fn, None,
                                                 fixed_key_below, C.c_void_p(l.ctypes.data), C.c_void_p(r.ctypes.data), C.c_void_p(fk.ctypes.data),
                                                 C.c_void_p(c.ctypes.data), rms, fms)
        if err:
            raise err[0]
        self.ctx.check(rc)
        out = (l[:lg], r[:lg], fk, c)
        return out + (list(rms)[:lg], list(fms)[:lg]) if want_times else out

    def ipa_round2_msms(self, coeffs_dev, n_quarter, u1):
        """Round 2's two commitments of an opening on this (committer) key by linearity (pc_hip_ipa_round2_msms): (l, r) affine."""
        u1 = np.ascontiguousarray(u1, dtype=np.uint64)
        w = 2 * FQ_BYTES[self.curve] // 8
        l, r = np.zeros(w, dtype=np.uint64), np.zeros(w, dtype=np.uint64)
        p, _ = _ptr(coeffs_dev)
        self.ctx.check(self.ctx.lib.pc_hip_ipa_round2_msms(self.ctx.h, self.h, p, n_quarter, C.c_void_p(u1.ctypes.data), C.c_void_p(l.ctypes.data), None,
                                                           C.c_void_p(r.ctypes.data), None))
        return l, r

    def fold2_from(self, n_quarter, u1, u2):
        """A new resident key of n_quarter points: the key after the first TWO folds (by u1, then u2), straight from this key
        (pc_hip_ec_fold2_from); self is left as it is."""
        u1 = np.ascontiguousarray(u1, dtype=np.uint64)
        u2 = np.ascontiguousarray(u2, dtype=np.uint64)
        h = C.c_void_p()
        self.ctx.check(self.ctx.lib.pc_hip_ec_fold2_from(self.ctx.h, self.h, n_quarter, C.c_void_p(u1.ctypes.data), C.c_void_p(u2.ctypes.data), C.byref(h)))
        out = Srs.__new__(Srs)
        out.ctx, out.curve, out.h, out.n = self.ctx, self.curve, h, n_quarter
        return out

    def fold_from(self, n_half, u):
        """A new resident key: affine(self[i] + u * self[n_half + i]), i < n_half; self is left as it is (pc_hip_ec_fold_from)."""
        u = np.ascontiguousarray(u, dtype=np.uint64)
        h = C.c_void_p()
        self.ctx.check(self.ctx.lib.pc_hip_ec_fold_from(self.ctx.h, self.h, n_half, C.c_void_p(u.ctypes.data), C.byref(h)))
        out = Srs.__new__(Srs)
        out.ctx, out.curve, out.h, out.n = self.ctx, self.curve, h, n_half
        return out

    def prefix(self, count):
        """A new resident key of the first `count` points, a device copy; this key is untouched (pc_hip_srs_prefix): trim's
        comm_key[0..count) (ipa_pc/mod.rs:384).  The new key has no window or fold table."""
        h = C.c_void_p()
        self.ctx.check(self.ctx.lib.pc_hip_srs_prefix(self.ctx.h, self.h, count, C.byref(h)))
        return Srs._adopt(self.ctx, self.curve, h, count)

    def check(self, offset=0, count=None, on_curve=True, subgroup=True, want_flags=False):
        """The check() of Validate::Yes over points [offset, offset + count) (pc_hip_srs_check): returns (bad, first_bad) -- how many
        points failed and the lowest failing index relative to offset (None when none failed) -- and with want_flags a third item,
        one byte per point, 1 for a point that passed."""
        return _key_check(self.ctx, self.ctx.lib.pc_hip_srs_check, self.h, self.n, offset, count, on_curve, subgroup, want_flags)

    def in_subgroup(self):
        """True if every point of the key lies in the prime-order subgroup (pc_hip_srs_in_subgroup; cached on the key)."""
        out = C.c_int(-1)
        self.ctx.check(self.ctx.lib.pc_hip_srs_in_subgroup(self.ctx.h, self.h, C.byref(out)))
        return bool(out.value)

    def device_ptr(self):
        """Address of the resident packed point array (pc_hip_srs_device_ptr)."""
        return int(self.ctx.lib.pc_hip_srs_device_ptr(self.h))

    def clone(self):
        """A second resident copy (device-to-device): what a destructive consumer -- the IPA key fold -- works on."""
        return Srs(self.ctx, self.curve, self.device_ptr(), n=self.n)

    def bytes_resident(self):
        out = (C.c_size_t * 4)()
        self.ctx.check(self.ctx.lib.pc_hip_srs_bytes_resident(self.h, out))
        return dict(zip(("bases", "window_tables", "fold_table", "pipelines"), [int(x) for x in out]))

    def serialize(self, offset=0, count=None, compressed=False):
        """ark-serialize bytes of resident points as a Vec<G1Affine> (pc_hip_srs_serialize)."""
        count = self.n - offset if count is None else count
        need = C.c_size_t()
        self.ctx.check(self.ctx.lib.pc_hip_srs_serialize(self.ctx.h, self.h, offset, count, 1 if compressed else 0, None, 0, C.byref(need)))
        buf = (C.c_char * need.value)()
        self.ctx.check(self.ctx.lib.pc_hip_srs_serialize(self.ctx.h, self.h, offset, count, 1 if compressed else 0, buf, need.value, C.byref(need)))
        return bytes(buf)

    def read(self, offset, count):
        out = np.zeros((count, 2 * FQ_BYTES[self.curve] // 8), dtype=np.uint64)
        self.ctx.check(self.ctx.lib.pc_hip_srs_read(self.ctx.h, self.h, offset, count, C.c_void_p(out.ctypes.data)))
        return out

    def msm_async(self, scalars, n=None, base_offset=0, montgomery=False):
        """Queue an MSM; returns a job whose .wait() gives (xy, is_infinity)."""
        p, where = _ptr(scalars)
        if n is None:
            n = scalars.shape[0]
        return MsmJob(self, p, where, n, base_offset, montgomery)


class G2Srs:
    """Resident G2 bases (pc_g2_srs): MultilinearPC's powers_of_h, or their pair sums.  Points are 192 bytes, x.c0 || x.c1 || y.c0 || y.c1."""

    def __init__(self, ctx, curve, bases, n=None, stride_bytes=0):
        self.ctx, self.curve = ctx, curve
        p, where = _ptr(bases)
        if n is None:
            n = bases.shape[0]
        h = C.c_void_p()
        ctx.check(ctx.lib.pc_hip_g2_srs_upload(ctx.h, CURVES[curve], p, n, stride_bytes, where, C.byref(h)))
        self.h, self.n = h, n

    @classmethod
    def _adopt(cls, ctx, curve, handle, n):
        """wrap a key the library made (pc_hip_ml_setup, pc_hip_ml_trim)"""
        out = cls.__new__(cls)
        out.ctx, out.curve, out.h, out.n = ctx, curve, handle, n
        return out

    def free(self):
        if self.h:
            self.ctx.lib.pc_hip_g2_srs_free(self.h)
            self.h = None

    def device_ptr(self):
        """Address of the resident packed point array (pc_hip_g2_srs_device_ptr)."""
        return int(self.ctx.lib.pc_hip_g2_srs_device_ptr(self.h))

    def __len__(self):
        return int(self.ctx.lib.pc_hip_g2_srs_len(self.h))

    def bytes_resident(self):
        out = (C.c_size_t * 4)()
        self.ctx.check(self.ctx.lib.pc_hip_g2_srs_bytes_resident(self.h, out))
        return dict(zip(("bases", "window_tables", "fold_table", "lanes"), [int(x) for x in out]))

    def read(self, offset, count):
        out = np.zeros((count, 4 * FQ_BYTES[self.curve]), dtype=np.uint8)
        self.ctx.check(self.ctx.lib.pc_hip_g2_srs_read(self.ctx.h, self.h, offset, count, C.c_void_p(out.ctypes.data)))
        return out

    def check(self, offset=0, count=None, on_curve=True, subgroup=True, want_flags=False):
        """Srs.check for a G2 key (pc_hip_g2_srs_check): the twist's equation and the plain ladder by r."""
        return _key_check(self.ctx, self.ctx.lib.pc_hip_g2_srs_check, self.h, self.n, offset, count, on_curve, subgroup, want_flags)

    def pair_sums_into(self, out_key, off, count, out_off):
        """out_key[out_off + b] = self[off + 2b] + self[off + 2b + 1], b < count (pc_hip_g2_srs_pair_sums)."""
        self.ctx.check(self.ctx.lib.pc_hip_g2_srs_pair_sums(self.ctx.h, self.h, off, count, out_key.h, out_off))

    def msm(self, scalars, n=None, base_offset=0, montgomery=False):
        """sum scalars[i] * bases[base_offset + i]; returns (192-byte uint8 array, is_infinity)."""
        p, where = _ptr(scalars)
        if n is None:
            n = scalars.shape[0]
        out = np.zeros(4 * FQ_BYTES[self.curve], dtype=np.uint8)
        inf = C.c_int(0)
        self.ctx.check(self.ctx.lib.pc_hip_g2_msm(self.ctx.h, self.h, base_offset, p,
                                                  PC_SCALARS_MONTGOMERY if montgomery else PC_SCALARS_CANONICAL,
                                                  where, n, C.c_void_p(out.ctypes.data), C.byref(inf)))
        return out, bool(inf.value)

    def ml_open(self, evals, nv, point):
        """MultilinearPC::open over this pair-sum key (pc_hip_ml_open): evals 2^nv Montgomery Fr (host array or device pointer), point nv
        Montgomery Fr (host).  Returns (nv x 192 bytes, nv infinity flags)."""
        p, where = _ptr(evals)
        point = np.ascontiguousarray(point)
        out = np.zeros((nv, 4 * FQ_BYTES[self.curve]), dtype=np.uint8)
        inf = (C.c_int * nv)()
        self.ctx.check(self.ctx.lib.pc_hip_ml_open(self.ctx.h, self.h, p, where, nv, C.c_void_p(point.ctypes.data), C.c_void_p(out.ctypes.data), inf))
        return out, [bool(x) for x in inf]


class TeSrs:
    """Resident twisted Edwards bases (pc_te_srs): the committer key of InnerProductArgPC over ed_on_bls12_381.  Points are 64 bytes,
    x || y in Montgomery form, on the way in and out; the identity is (0, ONE), there is no infinity."""

    def __init__(self, ctx, curve, bases, n=None, stride_bytes=0):
        self.ctx, self.curve = ctx, curve
        p, where = _ptr(bases)
        if n is None:
            n = bases.shape[0]
        h = C.c_void_p()
        ctx.check(ctx.lib.pc_hip_te_srs_upload(ctx.h, TE_CURVES[curve], p, n, stride_bytes, where, C.byref(h)))
        self.h, self.n = h, n

    @classmethod
    def _adopt(cls, ctx, curve, h, n):
        """a key object the library made (pc_hip_te_ec_fold_from)"""
        k = cls.__new__(cls)
        k.ctx, k.curve, k.h, k.n = ctx, curve, h, n
        return k

    def free(self):
        if self.h:
            self.ctx.lib.pc_hip_te_srs_free(self.h)
            self.h = None

    def __len__(self):
        return int(self.ctx.lib.pc_hip_te_srs_len(self.h))

    def bytes_resident(self):
        out = (C.c_size_t * 4)()
        self.ctx.check(self.ctx.lib.pc_hip_te_srs_bytes_resident(self.h, out))
        return dict(zip(("bases", "window_tables", "fold_table", "lanes"), [int(x) for x in out]))

    def read(self, offset, count):
        out = np.zeros((count, TE_POINT_BYTES[self.curve]), dtype=np.uint8)
        self.ctx.check(self.ctx.lib.pc_hip_te_srs_read(self.ctx.h, self.h, offset, count, C.c_void_p(out.ctypes.data)))
        return out

    def msm(self, scalars, n=None, base_offset=0, montgomery=False):
        """sum scalars[i] * bases[base_offset + i]; returns (64-byte uint8 array x || y, is_identity)."""
        p, where = _ptr(scalars)
        if n is None:
            n = scalars.shape[0]
        out = np.zeros(TE_POINT_BYTES[self.curve], dtype=np.uint8)
        ident = C.c_int(0)
        self.ctx.check(self.ctx.lib.pc_hip_te_msm(self.ctx.h, self.h, base_offset, p,
                                                  PC_SCALARS_MONTGOMERY if montgomery else PC_SCALARS_CANONICAL,
                                                  where, n, C.c_void_p(out.ctypes.data), C.byref(ident)))
        return out, bool(ident.value)

    def msm_many(self, scalars, m=None, n_msms=None, base_offset=0, montgomery=False):
        """n_msms MSMs of m pairs over bases[base_offset : base_offset + m] in one pass (pc_hip_te_msm_many; Hyrax's one commitment per
        matrix row).  scalars: (n_msms, m, 32) uint8 host array, or a device pointer / tensor with m and n_msms.
        Returns ((n_msms, 64) uint8 points x || y, (n_msms,) identity flags)."""
        p, where = _ptr(scalars)
        if m is None:
            n_msms, m = scalars.shape[0], scalars.shape[1]
        out = np.zeros((n_msms, TE_POINT_BYTES[self.curve]), dtype=np.uint8)
        ident = (C.c_int * max(n_msms, 1))()
        self.ctx.check(self.ctx.lib.pc_hip_te_msm_many(self.ctx.h, self.h, base_offset, p,
                                                       PC_SCALARS_MONTGOMERY if montgomery else PC_SCALARS_CANONICAL, where, m, n_msms,
                                                       C.c_void_p(out.ctypes.data), ident))
        return out, np.array(list(ident)[:n_msms], dtype=bool)

    def ec_fold(self, n_half, u_mont):
        """key[i] = key[i] + u * key[n_half + i], i < n_half, in place (pc_hip_te_ec_fold); u_mont: one Montgomery Fr (host, 32 bytes)."""
        u_mont = np.ascontiguousarray(u_mont)
        self.ctx.check(self.ctx.lib.pc_hip_te_ec_fold(self.ctx.h, self.h, n_half, C.c_void_p(u_mont.ctypes.data)))

    def ec_fold_from(self, n_half, u_mont):
        """A new resident key out[i] = key[i] + u * key[n_half + i], i < n_half; this key is untouched (pc_hip_te_ec_fold_from).  From the
        fold table when this key has one and n_half is half its length, by the ladder otherwise: the same points."""
        u_mont = np.ascontiguousarray(u_mont)
        h = C.c_void_p()
        self.ctx.check(self.ctx.lib.pc_hip_te_ec_fold_from(self.ctx.h, self.h, n_half, C.c_void_p(u_mont.ctypes.data), C.byref(h)))
        return TeSrs._adopt(self.ctx, self.curve, h, n_half)

    def prefix(self, count):
        """A new resident key of the first `count` points, a device copy; this key is untouched (pc_hip_te_srs_prefix): trim's
        comm_key[0..count)."""
        h = C.c_void_p()
        self.ctx.check(self.ctx.lib.pc_hip_te_srs_prefix(self.ctx.h, self.h, count, C.byref(h)))
        return TeSrs._adopt(self.ctx, self.curve, h, count)

    def precompute_fold(self):
        """Fold table of this (committer) key, once per key: 253 rows of its upper half and their doublings (pc_hip_te_srs_precompute_fold)."""
        self.ctx.check(self.ctx.lib.pc_hip_te_srs_precompute_fold(self.ctx.h, self.h))
        return self

    def fold_table_info(self):
        """rows of the fold table on this key; 0: none"""
        rows = C.c_uint()
        self.ctx.check(self.ctx.lib.pc_hip_te_srs_fold_table_info(self.h, C.byref(rows)))
        return rows.value

    def in_subgroup(self):
        """True if every point of the key lies in the prime-order subgroup (pc_hip_te_srs_in_subgroup; cached on the key)."""
        out = C.c_int(0)
        self.ctx.check(self.ctx.lib.pc_hip_te_srs_in_subgroup(self.ctx.h, self.h, C.byref(out)))
        return bool(out.value)

    def ipa_open_rounds(self, coeffs_dev, n, point_mont, h_prime_xy, next_challenge, fixed_key_below=0, want_times=False):
        """The whole halving loop of InnerProductArgPC::open on this resident committer key (pc_hip_te_ipa_open_rounds).
        next_challenge(l_xy, r_xy) (64 bytes each) -> u as 32 Montgomery bytes.  Returns (l_vec, r_vec, final_key, c[, round_ms, fold_ms])."""
        lg = n.bit_length() - 1
        pb = TE_POINT_BYTES[self.curve]
        l = np.zeros((max(lg, 1), pb), dtype=np.uint8)
        r = np.zeros((max(lg, 1), pb), dtype=np.uint8)
        fk, c = np.zeros(pb, dtype=np.uint8), np.zeros(32, dtype=np.uint8)
        err = []

        def cb(_user, lp, rp, up):
            try:
                lxy = np.frombuffer((C.c_uint8 * pb).from_address(lp), dtype=np.uint8).copy()
                rxy = np.frombuffer((C.c_uint8 * pb).from_address(rp), dtype=np.uint8).copy()
                u = np.ascontiguousarray(next_challenge(lxy, rxy), dtype=np.uint8)
                assert u.nbytes == 32
                C.memmove(up, u.ctypes.data, 32)
            except BaseException as e:      # an exception must not cross the C frames: finish the loop on a dummy challenge, raise afterwards
                err.append(e)
                C.memset(up, 0, 32); C.memset(up, 1, 1)
        fn = IPA_CHALLENGE_FN(cb)
        point = np.ascontiguousarray(point_mont)
        hp = np.ascontiguousarray(h_prime_xy)
        rms = (C.c_float * max(lg, 1))()
        fms = (C.c_float * max(lg, 1))()
        p, _ = _ptr(coeffs_dev)
        rc = self.ctx.lib.pc_hip_te_ipa_open_rounds(self.ctx.h, self.h, p, n, C.c_void_p(point.ctypes.data), C.c_void_p(hp.ctypes.data), fn, None,
                                                    fixed_key_below, C.c_void_p(l.ctypes.data), C.c_void_p(r.ctypes.data), C.c_void_p(fk.ctypes.data),
                                                    C.c_void_p(c.ctypes.data), rms, fms)
        if err:
            raise err[0]
        self.ctx.check(rc)
        out = (l[:lg], r[:lg], fk, c)
        return out + (list(rms)[:lg], list(fms)[:lg]) if want_times else out


def te_points_sum(curve, points):
    """Host-side sum of twisted Edwards points (k x 64 bytes) -> one point."""
    lib = load_library()
    points = np.ascontiguousarray(points)
    out = np.zeros(TE_POINT_BYTES[curve], dtype=np.uint8)
    rc = lib.pc_hip_te_points_sum(TE_CURVES[curve], C.c_void_p(points.ctypes.data), points.shape[0], C.c_void_p(out.ctypes.data))
    if rc != 0:
        raise PcHipError(rc, lib.pc_hip_strerror(rc).decode())
    return out


def te_point_mul(curve, point, scalar_mont):
    """Host-side k * P for one twisted Edwards point and one Montgomery-form Fr (the scalar as the integer it is)."""
    lib = load_library()
    point = np.ascontiguousarray(point)
    scalar_mont = np.ascontiguousarray(scalar_mont)
    out = np.zeros(TE_POINT_BYTES[curve], dtype=np.uint8)
    rc = lib.pc_hip_te_point_mul(TE_CURVES[curve], C.c_void_p(point.ctypes.data), C.c_void_p(scalar_mont.ctypes.data), C.c_void_p(out.ctypes.data))
    if rc != 0:
        raise PcHipError(rc, lib.pc_hip_strerror(rc).decode())
    return out


def ml_level_offset(nv, i):
    """points before level i in the keys of Context.ml_setup (level i holds 2^(nv - i) points)"""
    return (2 << nv) - (2 << (nv - i))


def multilinear_pair_key(ctx, curve, powers_of_h):
    """The pair-sum key of MultilinearPC::open: powers_of_h = nv host arrays (level i: 2^(nv - i) x 192 bytes).  Every level is uploaded,
    reduced to its pair sums on the device and dropped; the result holds 2^nv - 1 points, round i at offset 2^nv - 2^(nv - i)."""
    nv = len(powers_of_h)
    n = 1 << nv
    key = G2Srs(ctx, curve, np.zeros((n - 1, 4 * FQ_BYTES[curve]), dtype=np.uint8))
    for i, level in enumerate(powers_of_h):
        level = np.ascontiguousarray(level)
        assert level.shape[0] == n >> i
        lvl = G2Srs(ctx, curve, level)
        try:
            lvl.pair_sums_into(key, 0, n >> (i + 1), n - (n >> i))
        finally:
            lvl.free()
    return key


def g2_points_sum(curve, points):
    """Host-side sum of G2 affine points (k x 192 bytes) -> one point."""
    lib = load_library()
    points = np.ascontiguousarray(points)
    out = np.zeros(4 * FQ_BYTES[curve], dtype=np.uint8)
    rc = lib.pc_hip_g2_points_sum(CURVES[curve], C.c_void_p(points.ctypes.data), points.shape[0], C.c_void_p(out.ctypes.data))
    if rc != 0:
        raise PcHipError(rc, lib.pc_hip_strerror(rc).decode())
    return out


def g2_point_mul(curve, point, scalar_mont):
    """Host-side k * P for one G2 affine point and one Montgomery-form Fr."""
    lib = load_library()
    point = np.ascontiguousarray(point)
    scalar_mont = np.ascontiguousarray(scalar_mont)
    out = np.zeros(4 * FQ_BYTES[curve], dtype=np.uint8)
    rc = lib.pc_hip_g2_point_mul(CURVES[curve], C.c_void_p(point.ctypes.data), C.c_void_p(scalar_mont.ctypes.data), C.c_void_p(out.ctypes.data))
    if rc != 0:
        raise PcHipError(rc, lib.pc_hip_strerror(rc).decode())
    return out


class MsmJob:
    def __init__(self, srs, p, where, n, base_offset, montgomery):
        self.srs = srs
        self.out = np.zeros(2 * FQ_BYTES[srs.curve] // 8, dtype=np.uint64)
        self.inf = C.c_int(0)
        self.h = C.c_void_p()
        ctx = srs.ctx
        ctx.check(ctx.lib.pc_hip_msm_async(ctx.h, srs.h, base_offset, p,
                                           PC_SCALARS_MONTGOMERY if montgomery else PC_SCALARS_CANONICAL, where, n,
                                           C.c_void_p(self.out.ctypes.data), C.byref(self.inf), C.byref(self.h)))
        self.phases = None
        self.marks = None

    def wait(self):
        ctx = self.srs.ctx
        if self.h:
            ctx.check(ctx.lib.pc_hip_job_wait(ctx.h, self.h))
            self.h = None
            self.phases = ctx.last_msm_phases_ms()
            self.marks = ctx.last_msm_marks_ms()
        return self.out, bool(self.inf.value)


def universal_params_layout(curve, data, compressed):
    """Field offsets of a serialized kzg10::UniversalParams (pc_hip_universal_params_layout)."""
    lib = load_library()
    out = (C.c_size_t * 9)()
    buf = (C.c_char * len(data)).from_buffer_copy(data)
    rc = lib.pc_hip_universal_params_layout(CURVES[curve], buf, len(data), 1 if compressed else 0, out)
    if rc != 0:
        raise PcHipError(rc, lib.pc_hip_strerror(rc).decode())
    keys = ("powers_of_g", "n_powers_of_g", "powers_of_gamma_g", "n_powers_of_gamma_g", "h", "beta_h", "neg_powers_of_h", "n_neg_powers_of_h", "total")
    return dict(zip(keys, list(out)))


def points_sum(curve, points):
    """Host-side sum of affine points (k x 2*Fq uint64 array) -> one affine point."""
    lib = load_library()
    points = np.ascontiguousarray(points, dtype=np.uint64)
    out = np.zeros(2 * FQ_BYTES[curve] // 8, dtype=np.uint64)
    rc = lib.pc_hip_points_sum(CURVES[curve], C.c_void_p(points.ctypes.data), points.shape[0], C.c_void_p(out.ctypes.data))
    if rc != 0:
        raise PcHipError(rc, lib.pc_hip_strerror(rc).decode())
    return out


def point_mul(curve, point_xy, scalar_mont):
    """Host-side k * P for one affine point and one Montgomery-form Fr."""
    lib = load_library()
    point_xy = np.ascontiguousarray(point_xy, dtype=np.uint64)
    scalar_mont = np.ascontiguousarray(scalar_mont, dtype=np.uint64)
    out = np.zeros(2 * FQ_BYTES[curve] // 8, dtype=np.uint64)
    rc = lib.pc_hip_point_mul(CURVES[curve], C.c_void_p(point_xy.ctypes.data), C.c_void_p(scalar_mont.ctypes.data),
                              C.c_void_p(out.ctypes.data))
    if rc != 0:
        raise PcHipError(rc, lib.pc_hip_strerror(rc).decode())
    return out


class Group:
    """N single-device contexts driven from one process (pc_hip_group_*): one committer key sharded in contiguous
    chunks.  device_ids may repeat a device (tests on a one-GPU box)."""

    def __init__(self, device_ids):
        self.lib = load_library()
        ids = (C.c_int * len(device_ids))(*device_ids)
        h = C.c_void_p()
        rc = self.lib.pc_hip_group_create(ids, len(device_ids), C.byref(h))
        if rc != 0:
            raise PcHipError(rc, self.lib.pc_hip_strerror(rc).decode())
        self.h, self.n_dev = h, len(device_ids)

    def check(self, rc):
        if rc != 0:
            raise PcHipError(rc, self.lib.pc_hip_strerror(rc).decode())

    def close(self):
        if self.h:
            self.lib.pc_hip_group_destroy(self.h)
            self.h = None

    def upload_srs(self, curve, bases, precompute=False):
        return GroupSrs(self, curve, bases, precompute)

    def ntt_batch(self, curve, mat, log_n):
        mat = np.ascontiguousarray(mat, dtype=np.uint64)
        out = np.zeros((mat.shape[0], 1 << log_n, 4), dtype=np.uint64)
        self.check(self.lib.pc_hip_group_ntt_batch(self.h, CURVES[curve], mat.ctypes.data, mat.shape[0], mat.shape[1], log_n, out.ctypes.data))
        return out

    def ligero_commit(self, curve, mat, log_n, col_hash="blake2s", tree_hash="sha256", len_prefix=True):
        """LinearCodePCS::commit steps 1-3 with the rows split over the group's devices (pc_hip_group_ligero_commit): chained
        column digests, tree on the last device.  Returns (nodes (2^h - 1, 32) uint8 with the root at row 0, leaves (2^log_n, 32))."""
        mat = np.ascontiguousarray(mat, dtype=np.uint64)
        hid = {"sha256": 0, "blake2s": 1}
        nodes = np.zeros(((1 << max(1, log_n)) - 1, 32), dtype=np.uint8)
        leaves = np.zeros((1 << log_n, 32), dtype=np.uint8)
        self.check(self.lib.pc_hip_group_ligero_commit(self.h, CURVES[curve], mat.ctypes.data, mat.shape[0], mat.shape[1], log_n, hid[col_hash],
                                                       hid[tree_hash], 1 if len_prefix else 0, None, leaves.ctypes.data, nodes.ctypes.data))
        return nodes, leaves


class GroupJob:
    def __init__(self, gsrs, coeffs, z_mont, n, want_value=True):
        self.g = gsrs.g
        nq = 2 * FQ_BYTES[gsrs.curve] // 8
        self.comm, self.proof, self.val = np.zeros(nq, dtype=np.uint64), np.zeros(nq, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
        self.z = np.ascontiguousarray(z_mont, dtype=np.uint64)
        if isinstance(coeffs, np.ndarray):
            self.keep = np.ascontiguousarray(coeffs, dtype=np.uint64)
            ptr, where, n = C.c_void_p(self.keep.ctypes.data), PC_MEM_HOST, self.keep.shape[0]
        else:
            self.keep = (C.c_void_p * len(coeffs))(*coeffs)
            ptr, where = C.cast(self.keep, C.c_void_p), PC_MEM_DEVICE
        self.h = C.c_void_p()
        self.g.check(self.g.lib.pc_hip_group_commit_open_async(self.g.h, gsrs.h, ptr, where, n, self.z.ctypes.data, self.comm.ctypes.data,
                                                              self.proof.ctypes.data, self.val.ctypes.data if want_value else None, C.byref(self.h)))

    def wait(self):
        if self.h:
            self.g.check(self.g.lib.pc_hip_group_job_wait(self.g.h, self.h))
            self.h = None
        return self.comm, self.proof, self.val


class GroupSrs:
    def __init__(self, group, curve, bases, precompute=False):
        self.g, self.curve = group, curve
        bases = np.ascontiguousarray(bases, dtype=np.uint64)
        h = C.c_void_p()
        group.check(group.lib.pc_hip_group_srs_upload(group.h, CURVES[curve], bases.ctypes.data, bases.shape[0], 0, 1 if precompute else 0, C.byref(h)))
        self.h, self.n = h, bases.shape[0]

    def free(self):
        if self.h:
            self.g.lib.pc_hip_group_srs_free(self.h)
            self.h = None

    def msm(self, scalars, base_offset=0, montgomery=False):
        scalars = np.ascontiguousarray(scalars, dtype=np.uint64)
        out = np.zeros(2 * FQ_BYTES[self.curve] // 8, dtype=np.uint64)
        inf = C.c_int(0)
        self.g.check(self.g.lib.pc_hip_group_msm(self.g.h, self.h, base_offset, scalars.ctypes.data,
                                                 PC_SCALARS_MONTGOMERY if montgomery else PC_SCALARS_CANONICAL, scalars.shape[0],
                                                 out.ctypes.data, C.byref(inf)))
        return out, bool(inf.value)

    def msm_batch(self, polys, montgomery=True):
        polys = [np.ascontiguousarray(p, dtype=np.uint64) for p in polys]
        k = len(polys)
        ptrs = (C.c_void_p * k)(*[p.ctypes.data for p in polys])
        ns = (C.c_size_t * k)(*[p.shape[0] for p in polys])
        out = np.zeros((k, 2 * FQ_BYTES[self.curve] // 8), dtype=np.uint64)
        self.g.check(self.g.lib.pc_hip_group_msm_batch(self.g.h, self.h, ptrs, ns, k, PC_SCALARS_MONTGOMERY if montgomery else PC_SCALARS_CANONICAL,
                                                       out.ctypes.data, None))
        return out

    def commit_open_async(self, coeffs, z_mont, n=None, want_value=True):
        """pc_hip_group_commit_open_async: coeffs = host (n, 4) uint64 array (Montgomery), or a list of N device pointers with `n`.
        Returns a job; job.wait() -> (commitment xy, proof xy, p(z))."""
        return GroupJob(self, coeffs, z_mont, n, want_value)

    def kzg_open(self, coeffs_mont, z_mont):
        coeffs_mont = np.ascontiguousarray(coeffs_mont, dtype=np.uint64)
        z_mont = np.ascontiguousarray(z_mont, dtype=np.uint64)
        out = np.zeros(2 * FQ_BYTES[self.curve] // 8, dtype=np.uint64)
        val = np.zeros(4, dtype=np.uint64)
        inf = C.c_int(0)
        self.g.check(self.g.lib.pc_hip_group_kzg_open(self.g.h, self.h, coeffs_mont.ctypes.data, coeffs_mont.shape[0], z_mont.ctypes.data,
                                                      out.ctypes.data, C.byref(inf), val.ctypes.data))
        return out, val
