#!/usr/bin/env python3
"""Regenerate rust/poly-commit-hip/src/ffi.rs from include/pc_hip.h (types mapped by tools/check_ffi_decls.py).
Every function of the header must be listed in GROUPS below (the script refuses to write otherwise), so a new entry point
is placed, with its reference citation, by whoever adds it."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import check_ffi_decls as c  # noqa: E402

KW = {"in": "input", "where": "where_"}
GROUPS = [
    ("Library / device lifetime", ["pc_hip_device_count", "pc_hip_init", "pc_hip_shutdown", "pc_hip_strerror", "pc_hip_last_error"]),
    ("SRS residency: the hook of MarlinKZG10::trim (marlin_pc/mod.rs:80-169, powers copied at :96) and InnerProductArgPC::trim (ipa_pc/mod.rs:359-401)",
     ["pc_hip_srs_upload", "pc_hip_srs_free", "pc_hip_srs_load_serialized", "pc_hip_srs_serialize", "pc_hip_universal_params_layout", "pc_hip_srs_precompute", "pc_hip_srs_precompute_ex", "pc_hip_srs_len", "pc_hip_srs_device_ptr", "pc_hip_srs_read",
      "pc_hip_srs_bytes_resident", "pc_hip_ctx_bytes_resident", "pc_hip_ctx_trim"]),
    ("<E::G1 as VariableBaseMSM>::msm_bigint: kzg10/mod.rs:175-178, :255-258; ipa_pc/mod.rs:64; the loop of MarlinKZG10::commit (marlin_pc/mod.rs:192-237); HyraxPC::commit's rows (hyrax/mod.rs:233-242)",
     ["pc_hip_msm", "pc_hip_msm_batch", "pc_hip_msm_async", "pc_hip_job_wait", "pc_hip_msm_many"]),
    ("device buffers for a caller that links no HIP runtime itself", ["pc_hip_malloc", "pc_hip_free", "pc_hip_memcpy_h2d", "pc_hip_memcpy_d2h"]),
    ("compute_witness_polynomial (kzg10/mod.rs:217-240), KZG10::open as one call (:287-310), Polynomial::evaluate, the open-side combination (marlin_pc/mod.rs:281-287)",
     ["pc_hip_witness_poly", "pc_hip_kzg_open", "pc_hip_poly_eval", "pc_hip_poly_div_scan", "pc_hip_fr_lincomb"]),
    ("host-side point utilities (kzg10/mod.rs:206; ipa_pc/mod.rs:672,675)", ["pc_hip_points_sum", "pc_hip_point_mul"]),
    ("InnerProductArgPC::open's halving loop on device-resident vectors (ipa_pc/mod.rs:641-711), the verifier's check polynomial (:759-765)",
     ["pc_hip_fr_fold", "pc_hip_fr_dot", "pc_hip_ipa_fold_dots", "pc_hip_fr_powers", "pc_hip_ec_fold", "pc_hip_ec_fold_from", "pc_hip_ec_fold2_from", "pc_hip_ipa_round2_msms", "pc_hip_ipa_open_rounds", "pc_hip_srs_precompute_fold", "pc_hip_srs_precompute_fold_ex", "pc_hip_srs_fold_table_info", "pc_hip_ipa_key_scalars"]),
    ("KZG10::setup's g.batch_mul(&powers_of_beta) (kzg10/mod.rs:76,83)", ["pc_hip_fixed_base_batch_mul"]),
    ("Ligero: reed_solomon over every row (linear_codes/utils.rs:112-127, mod.rs:131-135), column digests (:256-263), Merkle tree (:270-274, :506-521), queried columns (:546-552)",
     ["pc_hip_ntt_batch", "pc_hip_column_hash", "pc_hip_column_hash_part", "pc_hip_merkle_tree", "pc_hip_matrix_columns", "pc_hip_ligero_commit"]),
    ("Brakedown: the resident code (BrakedownPCParams' matrices, brakedown.rs:146-203), MultilinearBrakedown::encode over every row (multilinear_brakedown/mod.rs:56-84), commit steps 1-3 (linear_codes/mod.rs:248-277)",
     ["pc_hip_brakedown_code_create", "pc_hip_brakedown_code_free", "pc_hip_brakedown_codeword_len", "pc_hip_brakedown_encode", "pc_hip_brakedown_commit"]),
    ("G2 and MultilinearPC: <E::G2 as VariableBaseMSM>::msm_bigint (multilinear_pc/mod.rs:162-163), the halving rounds of open (:153-157), open as one call (:131-168), the key's residency (trim, :91-111)",
     ["pc_hip_g2_srs_upload", "pc_hip_g2_srs_free", "pc_hip_g2_srs_len", "pc_hip_g2_srs_bytes_resident", "pc_hip_g2_srs_pair_sums", "pc_hip_g2_srs_read", "pc_hip_g2_msm",
      "pc_hip_g2_points_sum", "pc_hip_g2_point_mul", "pc_hip_ml_fold", "pc_hip_ml_open"]),
    ("MultilinearPC::setup on the device: the eq tables (multilinear_pc/mod.rs:36-51, 219-234), g.batch_mul / h.batch_mul (:60-62) as level 0 and pair sums, g_mask (:75); trim from the resident parameters (:91-111)",
     ["pc_hip_ml_eq_evals", "pc_hip_g2_fixed_base_batch_mul", "pc_hip_g2_srs_device_ptr", "pc_hip_ml_setup", "pc_hip_ml_trim"]),
    ("streaming_kzg: FoldedPolynomialTree (streaming_kzg/data_structures.rs:12-138), open_multi_points (space.rs:98-136, time.rs:126-137), batch_open_multi_points (time.rs:141-152), commit_folding / open_folding (space.rs:165-262)",
     ["pc_hip_fold_tree", "pc_hip_poly_div_multi", "pc_hip_kzg_open_multi", "pc_hip_kzg_batch_open_multi", "pc_hip_kzg_commit_folding", "pc_hip_kzg_open_folding"]),
    ("MarlinPST13 in the dense lexicographic layout: powers_of_beta of setup (marlin_pst13_pc/mod.rs:187-207), divide_at_point (:44-92), commit (:353-362), open (:419-512), trim's selection (:283-288); the layout helpers sort a BTreeMap key into device order",
     ["pc_hip_pst13_key_len", "pc_hip_pst13_rank", "pc_hip_pst13_unrank", "pc_hip_pst13_monomial_evals", "pc_hip_pst13_scatter", "pc_hip_pst13_divide", "pc_hip_pst13_commit",
      "pc_hip_pst13_open", "pc_hip_pst13_trim"]),
    ("InnerProductArgPC over the twisted Edwards curve ed_on_bls12_381, the reference's own instantiation (ipa_pc/mod.rs:1056-1064): cm_commit's msm_bigint (:54-72), the key fold of open (:699-707), the key's residency (trim, :359-401)",
     ["pc_hip_te_srs_upload", "pc_hip_te_srs_free", "pc_hip_te_srs_len", "pc_hip_te_srs_read", "pc_hip_te_srs_bytes_resident", "pc_hip_te_msm", "pc_hip_te_ec_fold",
      "pc_hip_te_points_sum", "pc_hip_te_point_mul"]),
    ("InnerProductArgPC::open over ed_on_bls12_381 on the device: the vectors of the halving rounds over the 252-bit scalar field (ipa_pc/mod.rs:641-649, 672-697), the out-of-place key fold and its table (:699-707), the subgroup fact that sample_generators establishes (:320), the rounds as one call (:664-711)",
     ["pc_hip_te_fr_powers", "pc_hip_te_ipa_fold_dots", "pc_hip_te_ipa_key_scalars", "pc_hip_te_ec_fold_from", "pc_hip_te_srs_precompute_fold", "pc_hip_te_srs_fold_table_info",
      "pc_hip_te_srs_in_subgroup", "pc_hip_te_ipa_open_rounds"]),
    ("InnerProductArgPC::setup and trim over ed_on_bls12_381 on the device (ipa_pc/mod.rs:302-325, 344-400): sample_generators -- Blake2s, from_random_bytes with its square root, the cofactor, normalize_batch -- as a new resident key, and trim's prefix of it",
     ["pc_hip_te_sample_generators", "pc_hip_te_srs_prefix"]),
    ("InnerProductArgPC::setup and trim (ipa_pc/mod.rs:302-325, 344-400) and HyraxPC::setup (hyrax/mod.rs:119-168) over the short Weierstrass curves on the device: sample_generators -- Blake2s, short_weierstrass from_random_bytes with its square root, mul_by_cofactor_to_group, normalize_batch -- as a new resident key, and trim's prefix of it",
     ["pc_hip_sample_generators", "pc_hip_srs_prefix"]),
    ("HyraxPC over ed_on_bls12_381, the reference's Hyrax381 (hyrax/tests.rs:6,20-21): commit's Pedersen commitment per matrix row as one many-MSM pass over a window table of the key (hyrax/mod.rs:86-93, 233-242), and the vectors of open over the 252-bit scalar field -- row_mul (:347, :391) and the inner product (:356)",
     ["pc_hip_te_msm_many", "pc_hip_te_fr_lincomb", "pc_hip_te_fr_dot"]),
    ("one committer key over the GPUs of a node, one process",
     ["pc_hip_group_create", "pc_hip_group_destroy", "pc_hip_group_size", "pc_hip_group_ctx", "pc_hip_group_srs_upload", "pc_hip_group_srs_free",
      "pc_hip_group_srs_len", "pc_hip_group_msm", "pc_hip_group_msm_batch", "pc_hip_group_kzg_open", "pc_hip_group_commit_open_async", "pc_hip_group_job_wait", "pc_hip_group_ntt_batch", "pc_hip_group_ligero_commit"]),
    ("measurement and tuning hooks (bench.py, tests); a prover does not need them",
     ["pc_hip_set_msm_tuning", "pc_hip_set_timing", "pc_hip_last_msm_phases_ms", "pc_hip_last_msm_marks_ms", "pc_hip_last_msm_shape",
      "pc_hip_last_ntt_phases_ms", "pc_hip_last_ligero_phases_ms", "pc_hip_last_brakedown_phases_ms", "pc_hip_last_skzg_launches", "pc_hip_last_pst13_shape"]),
]
HEAD = '''//! Raw declarations of the C ABI of `libpc_hip.so` (`include/pc_hip.h`): one `extern "C"` symbol per call the shim
//! replaces in the reference.  GENERATED by tools/gen_ffi_rs.py from the header; `tools/check_ffi_decls.py` (run by the
//! repo's CPU test suite) parses the header and this file and fails on any missing function, arity or type mismatch, or
//! constant that differs.
#![allow(non_camel_case_types, dead_code)]
use core::ffi::{c_char, c_int, c_uint, c_void};

macro_rules! opaque { ($($n:ident),*) => { $( #[repr(C)] pub struct $n { _p: [u8; 0], _m: core::marker::PhantomData<(*mut u8, core::marker::PhantomPinned)> } )* } }
opaque!(pc_ctx, pc_srs, pc_job, pc_lincode, pc_g2_srs, pc_te_srs, pc_group, pc_group_srs, pc_group_job);

/// `pc_ipa_challenge_fn`: the caller's transcript inside `pc_hip_ipa_open_rounds` (user, l, r -> u; points as x || y, u as Montgomery limbs)
pub type pc_ipa_challenge_fn = Option<unsafe extern "C" fn(user: *mut c_void, l_xy: *const c_void, r_xy: *const c_void, out_u_mont: *mut c_void)>;
'''


def main():
    funcs, enums, defs = c.parse_header()
    listed = [n for _, ns in GROUPS for n in ns]
    missing = [n for n in funcs if n not in listed]
    stale = [n for n in listed if n not in funcs]
    if missing or stale:
        raise SystemExit(f"gen_ffi_rs: place these in GROUPS: {missing}; no longer in the header: {stale}")
    out = [HEAD]

    def const_block(title, keys):
        return f"// {title}\n" + "".join(f"pub const {k}: c_int = {enums[k] if k in enums else defs[k]};\n" for k in keys)
    out.append(const_block("pc_curve", ["PC_CURVE_BLS12_381", "PC_CURVE_BN254", "PC_CURVE_PALLAS", "PC_CURVE_BLS12_377"]))
    out.append(const_block("pc_te_curve: the twisted Edwards curves (an id space of their own)", ["PC_TE_ED_ON_BLS12_381"]))
    out.append(const_block("pc_scalar_form: CANONICAL = &[F::BigInt] (msm_bigint's argument); MONTGOMERY = &[F] as poly.coeffs() lies in memory",
                           ["PC_SCALARS_CANONICAL", "PC_SCALARS_MONTGOMERY"]))
    out.append(const_block("pc_mem", ["PC_MEM_HOST", "PC_MEM_DEVICE"]))
    out.append(const_block("pc_hash", ["PC_HASH_SHA256", "PC_HASH_BLAKE2S"]))
    out.append(const_block("pc_status", ["PC_OK", "PC_ERR_INVALID_ARG", "PC_ERR_OOM", "PC_ERR_HIP", "PC_ERR_NO_DEVICE", "PC_ERR_TOO_LARGE", "PC_ERR_UNSUPPORTED", "PC_ERR_INTERNAL"]))
    out.append(const_block("limits", sorted(defs)))
    out.append('#[link(name = "pc_hip")]\nextern "C" {')
    for title, names in GROUPS:
        out.append(f"    // ---- {title}")
        for name in names:
            args, ret = funcs[name]
            parts = [f"{KW.get(n, n)}: {t}" for n, t in args]
            tail = ")" + (f" -> {ret};" if ret != "()" else ";")
            line = f"    pub fn {name}(" + ", ".join(parts) + tail
            if len(line) > 130:
                lines, cur = [], f"    pub fn {name}("
                for i, p in enumerate(parts):
                    piece = p + (", " if i + 1 < len(parts) else "")
                    if len(cur) + len(piece) > 125:
                        lines.append(cur.rstrip()); cur = "        " + piece
                    else:
                        cur += piece
                lines.append(cur.rstrip() + tail)
                line = "\n".join(lines)
            out.append(line)
    out.append("}")
    with open(c.FFI_RS, "w") as f:
        f.write("\n".join(out) + "\n")
    print(f"wrote {c.FFI_RS}: {len(funcs)} functions")


if __name__ == "__main__":
    main()
