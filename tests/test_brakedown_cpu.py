"""CPU suite of the Brakedown linear code: the Python restatement (tests/harness/brakedown.py), the C++ host mirror
(poly_commit_amd/host/brakedown.hpp through tests/cpp/brakedown_driver.cpp) and the kernel bodies of csrc/sprs.hpp stepped lane by
lane (tests/emu/emu_brakedown.cpp) against each other, against the reference's own row_mul vectors and against the restated table of
default dimensions (tests/golden/brakedown.json).  All comparisons are exact."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from harness import brakedown as B
from harness.brakedown import FIELD_ID, driver, flat_arrays, malformed, messages

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CURVES = ["bls12_381", "bn254", "pallas"]
GOLDEN = json.load(open(os.path.join(HERE, "golden", "brakedown.json")))
_emu = None


def emu():
    global _emu
    if _emu is None:
        so = os.path.join(HERE, "emu", "libemu_brakedown.so")
        srcs = [os.path.join(HERE, "emu", "emu_brakedown.cpp")] + [os.path.join(ROOT, "poly_commit_amd", "csrc", f) for f in ("sprs.hpp", "fp32.hpp")]
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(s) for s in srcs):
            tmp = "%s.%d.tmp" % (so, os.getpid())
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", tmp, srcs[0]])
            os.replace(tmp, so)
        _emu = C.CDLL(so)
        sz, vp = C.c_size_t, C.c_void_p
        _emu.emu_brakedown_validate.argtypes = [sz, sz, sz, vp, vp, vp, sz]
        _emu.emu_brakedown_encode.argtypes = [C.c_int, sz, sz, sz, vp, vp, vp, vp, sz, vp, C.c_uint32, vp]
    return _emu


def emu_validate(msg_len, m_ext, dims, ind_ptr, col_ind):
    return emu().emu_brakedown_validate(msg_len, m_ext, len(dims) // 6, dims.ctypes.data, ind_ptr.ctypes.data, col_ind.ctypes.data, len(col_ind))


def emu_encode(code, msgs):
    """msgs: rows lists of canonical integers -> rows lists of canonical integers, through the stepped kernel bodies."""
    dims, ind_ptr, col_ind, val = flat_arrays(code)
    m = B.monts(code.curve, [x for row in msgs for x in row])
    out = np.zeros((len(msgs) * code.m_ext, 4), dtype=np.uint64)
    rc = emu().emu_brakedown_encode(FIELD_ID[code.curve], code.m, code.m_ext, len(dims) // 6, dims.ctypes.data, ind_ptr.ctypes.data, col_ind.ctypes.data,
                                    val.ctypes.data, len(col_ind), m.ctypes.data, len(msgs), out.ctypes.data)
    assert rc == 0, rc
    # canonical residues: the column hash absorbs these bytes
    raw = [int.from_bytes(out[i].tobytes(), "little") for i in range(out.shape[0])]
    assert all(x < code.p for x in raw)
    got = B.ints(code.curve, out)
    return [got[r * code.m_ext:(r + 1) * code.m_ext] for r in range(len(msgs))]


# ---- 1. row_mul vectors and default dimensions -------------------------------------------------------------------------------------------
def test_row_mul_reference_vectors_and_default_dimensions():
    g = GOLDEN["row_mul"]
    p = B.field_p("bls12_381")
    flat, n, m = g["flat_column_major"], g["n"], g["m"]
    cols = [[(i, flat[j * n + i]) for i in range(n)] for j in range(m)]
    assert B.SprsMat.new_from_flat(n, m, g["d"], flat).row_mul(g["v"], p) == g["result"]
    assert B.SprsMat.new_from_columns(n, m, g["d"], cols).row_mul(g["v"], p) == g["result"]
    exe = driver()
    assert "rowmul OK" in subprocess.run([exe, "rowmul"], capture_output=True, text=True, timeout=60, check=True).stdout
    lines = subprocess.run([exe, "table"], capture_output=True, text=True, timeout=60, check=True).stdout.strip().splitlines()
    assert len(lines) == 10
    table = {row["num_vars"]: row for row in GOLDEN["default_dimensions"]}
    assert sorted(table) == [10, 12, 16, 20, 24]
    seen = set()
    for ln in lines:
        head, a, b = [x.strip() for x in ln.split("|")]
        bits, nv, n, m, m_ext = [int(x) for x in head.split()]
        a_dims = [tuple(int(y) for y in x.split(",")) for x in a.split()]
        b_dims = [tuple(int(y) for y in x.split(",")) for x in b.split()]
        py = B.default_shape(1 << nv, bits)
        want = table[nv]
        assert py == (n, m, a_dims, b_dims, m_ext), (bits, nv)
        assert (want["n"], want["m"], [tuple(x) for x in want["a_dims"]], [tuple(x) for x in want["b_dims"]], want["m_ext"]) == py, (bits, nv)
        assert sum(x[0] * x[2] for x in a_dims + b_dims) == want["nnz"]
        # the conditions the encoder's schedule rests on
        code = B.Code("bn254", m, a_dims, b_dims, [], [])
        assert all(a_dims[i + 1][0] == a_dims[i][1] for i in range(len(a_dims) - 1))
        assert all(code.end[i] - code.start[i] == b_dims[i][0] for i in range(len(b_dims)))
        seen.add((bits, nv))
    assert len(seen) == 10


# ---- 2. make_mat ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve,n,m,d", [("bn254", 92, 17, 10), ("bls12_381", 140, 127, 19), ("pallas", 65, 12, 8)])
def test_make_mat_same_in_python_and_cpp(curve, n, m, d, tmp_path):
    p = B.field_p(curve)
    mat = B.make_mat(n, m, d, B.Gen(0xBD0 + n), p)
    out = tmp_path / "mat.bin"
    r = subprocess.run([driver(), "makemat", str(FIELD_ID[curve]), str(n), str(m), str(d), str(0xBD0 + n), str(out)], capture_output=True, text=True, timeout=60, check=True)
    nnz = int(r.stdout.split()[1])
    raw = out.read_bytes()
    assert nnz == n * d == len(mat.val) and len(raw) == 8 * (m + 1) + 8 * nnz + 32 * nnz
    ind_ptr = np.frombuffer(raw, dtype="<u8", count=m + 1).tolist()
    col_ind = np.frombuffer(raw, dtype="<u8", count=nnz, offset=8 * (m + 1)).tolist()
    val = B.ints(curve, np.frombuffer(raw, dtype="<u8", offset=8 * (m + 1) + 8 * nnz).reshape(-1, 4))
    assert (ind_ptr, col_ind, val) == (mat.ind_ptr, mat.col_ind, mat.val)
    per_row = [0] * n
    for i in col_ind:
        per_row[i] += 1
    assert per_row == [d] * n and all(0 < v < p for v in val)
    for j in range(m):                                          # a row appears at most once in a column
        rows = col_ind[ind_ptr[j]:ind_ptr[j + 1]]
        assert len(set(rows)) == len(rows)


# ---- 3. systematic, linear ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["nv10", "nv12", "m17"])
def test_encode_is_linear_and_systematic_where_the_reference_is(which):
    """With levels the codeword starts with the message.  With a_dims empty (m = 17 < base_len) the reference's encode is the base
    code ALONE: naive_reed_solomon(cw, 0, m, m_ext) overwrites cw[0..m_ext) (mod.rs:73-76), so that code is not systematic -- position
    k holds the message polynomial's value at k + 1; this is what is asserted for it."""
    curve = "bn254"
    code = B.base_code(curve, 17) if which == "m17" else B.default_code(curve, int(which[2:]), 0x5EED)[1]
    p = code.p
    x, y = messages(code, 2, 31)
    a, b = B.Gen(77).nonzero(p), B.Gen(78).nonzero(p)
    ex, ey = B.encode(code, x), B.encode(code, y)
    assert len(ex) == code.m_ext
    if which == "m17":
        assert code.m_ext == B.ceil_mul(17, B.RHO_INV) == 26
        assert ex == [sum(c * pow(k, i, p) for i, c in enumerate(x)) % p for k in range(1, 27)]
    else:
        assert ex[:code.m] == x and ey[:code.m] == y
    assert B.encode(code, [(a * u + b * v) % p for u, v in zip(x, y)]) == [(a * u + b * v) % p for u, v in zip(ex, ey)]


# ---- 4. the reference's loop order ----------------------------------------------------------------------------------------------------------
def test_loop_order_of_the_b_products_is_the_references():
    """mod.rs:79-82 runs level 0 first.  Reversing the loop gives another codeword; the clipped concurrent form (what the device
    launches) equals the loop as written in ANY order; the unclipped form in reversed order does not.  The C++ mirror's host encode
    and the stepped kernels agree with the loop as written."""
    curve = "bn254"
    _, code = B.default_code(curve, 12, 0xC0DE)
    msg = messages(code, 1, 5)[0]
    want = B.encode(code, msg)
    levels = list(range(len(code.start)))
    rev = B.encode(code, msg, b_order=levels[::-1])
    assert sum(u != v for u, v in zip(want, rev)) == 593              # of 3116, for this seed (DESIGN.md 4b quotes it)
    for order in (levels, levels[::-1], [1, 2, 0]):
        assert B.encode(code, msg, b_order=order, clip=True) == want
    assert B.encode(code, msg, b_order=levels[::-1], clip=False) != want
    assert emu_encode(code, [msg])[0] == want


@pytest.mark.parametrize("curve", CURVES)
def test_cpp_mirror_host_encode_equals_the_restatement(curve, tmp_path):
    nv, seed = 10, 0xFACE
    n, code = B.default_code(curve, nv, seed)
    out = tmp_path / "cw.bin"
    subprocess.run([driver(), "encode", str(FIELD_ID[curve]), str(nv), str(seed), "0", str(out)], capture_output=True, text=True, timeout=120, check=True)
    got = B.ints(curve, np.frombuffer(out.read_bytes(), dtype="<u8").reshape(-1, 4))
    g = B.Gen(seed + 1)
    msgs = [[g.nonzero(code.p) for _ in range(code.m)] for _ in range(n)]
    assert got == [x for row in msgs for x in B.encode(code, row)]


# ---- 5. the kernel bodies, stepped ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("nv", [10, 12])
@pytest.mark.parametrize("rows", [1, 2, 3, 64, 65])
def test_stepped_kernels_default_codes(curve, nv, rows):
    """rows 64 and 65 are the wave-boundary cases of the lane = (column, row) packing.  (This steps the bodies' indexing and the
    schedule with the host forms of the field arithmetic; the device's fused multiplier is covered by the GPU tests.)"""
    _, code = B.default_code(curve, nv, 0xE0 + nv)
    msgs = messages(code, rows, 100 + rows)
    assert emu_encode(code, msgs) == [B.encode(code, m) for m in msgs], (curve, nv, rows)


@pytest.mark.parametrize("curve", CURVES)
def test_stepped_kernels_ragged_and_base_codes(curve):
    rc = B.ragged_code(curve)
    mats = rc.a_mats + rc.b_mats
    lens = [[mt.ind_ptr[j + 1] - mt.ind_ptr[j] for j in range(mt.m)] for mt in mats]
    assert any(0 in x for x in lens) and any(mt.n in x for mt, x in zip(mats, lens)) and mats[1].d == 1      # empty column, full column, d = 1
    for code in (rc, B.base_code(curve, 17), B.base_code(curve, 29, 61)):
        for rows in (1, 2, 3, 64, 65):
            msgs = messages(code, rows, 300 + rows)
            assert emu_encode(code, msgs) == [B.encode(code, m) for m in msgs], (curve, code.m, rows)


# ---- 6. ABI ------------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_exported_and_null_arguments_need_no_device():
    import poly_commit_amd as pc
    driver()
    lib = pc.load_library()
    for s in ("pc_hip_brakedown_code_create", "pc_hip_brakedown_code_free", "pc_hip_brakedown_codeword_len", "pc_hip_brakedown_encode",
              "pc_hip_brakedown_commit", "pc_hip_last_brakedown_phases_ms"):
        assert hasattr(lib, s), s
    h = C.c_void_p()
    assert lib.pc_hip_brakedown_code_create(None, 1, 17, 26, 0, None, None, None, None, 0, C.byref(h)) == -1 and not h.value
    assert lib.pc_hip_brakedown_code_create(None, 1, 17, 26, 0, None, None, None, None, 0, None) == -1
    assert lib.pc_hip_brakedown_encode(None, None, None, 0, 1, None, 0) == -1
    assert lib.pc_hip_brakedown_commit(None, None, None, 0, 1, 1, 0, 1, None, 0, None, None) == -1
    assert lib.pc_hip_last_brakedown_phases_ms(None, None) == -1
    assert lib.pc_hip_brakedown_codeword_len(None) == 0
    lib.pc_hip_brakedown_code_free(None)


def test_array_checks_reject_malformed_codes_on_the_host():
    """brakedown_validate (csrc/sprs.hpp) is what pc_hip_brakedown_code_create calls before it touches the device."""
    for nv in (10, 12):
        _, code = B.default_code("bn254", nv, 0xAB + nv)
        dims, ind_ptr, col_ind, _ = flat_arrays(code)
        assert emu_validate(code.m, code.m_ext, dims, ind_ptr, col_ind) == 0
        for name, dm, ip, ci, m_ext in malformed(code):
            assert emu_validate(code.m, m_ext, dm, ip, ci) != 0, (nv, name)
    rc = B.ragged_code("pallas")
    assert emu_validate(rc.m, rc.m_ext, *flat_arrays(rc)[:3]) == 0
    none = np.zeros(0, dtype=np.uintp)
    assert emu_validate(17, 26, none, none, none.astype(np.uint32)) == 0 and emu_validate(17, 16, none, none, none.astype(np.uint32)) != 0
