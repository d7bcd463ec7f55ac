"""The C-ABI of include/tfk.h as exported by the CPU restatement (oracle/oracle_tfk.c, host pointers, stream = NULL;
SURVEY.md 8(b)): the same ctypes call sequence a reference-side binding would make against libtfk.so, here run on the
host against the REFERENCE's golden outputs -- and that libtfk.so itself exports every symbol the header declares
(no compute calls without a GPU), bound by a table (``native.bind``) that agrees with every prototype of the header."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_vp, _f = C.c_void_p, C.c_float


def rel(a, b):
    return float(np.nanmax(np.abs(np.asarray(a, np.float64) - b) / np.maximum(1.0, np.abs(b))))


def ptr(a):
    return a.ctypes.data_as(_vp) if a is not None else None


@pytest.fixture(scope="module")
def cpu_abi(oracle):
    """The CPU restatement, bound from the same table as libtfk.so (the symbols it exports)."""
    from torchflows_amd import native
    L = C.CDLL(oracle.build())
    native.bind(L, [s for s in native.SYMBOLS if hasattr(L, s)])
    return L


# ---- the binding table against the header's text -------------------------------------------------------------------
_STRUCTURES = {"tfk_glow_layer": "GlowLayer", "tfk_glow_level_step": "GlowLevelStep",
               "tfk_convnet_train_plan": "ConvNetTrainPlan"}


def _ctype_class(t, native):
    """The class of tests/tfk_header.py a ctypes type stands for."""
    if t is None:
        return None
    if t in (C.c_void_p, C.c_char_p):
        return "ptr"
    if isinstance(t, type) and issubclass(t, C._Pointer):
        for cname, pyname in _STRUCTURES.items():
            if t._type_ is getattr(native, pyname):
                return "ptr:" + cname
        return "ptr"
    if isinstance(t, type) and issubclass(t, C.Structure):
        for cname, pyname in _STRUCTURES.items():
            if t is getattr(native, pyname):
                return "struct:" + cname
    return {C.c_int32: "i32", C.c_int64: "i64", C.c_float: "f32"}[t]


def _same_class(bound: str, declared: str) -> bool:
    # a pointer to one of the header's structs is bound as POINTER(<its structure>), or as void * where the caller passes byref
    return bound == declared or (declared.startswith("ptr:") and bound == "ptr")


def test_binding_table_matches_every_prototype():
    """Every function include/tfk.h declares has a row in native's table with the same number of parameters, the same
    class (struct pointer / pointer / int32 / int64 / float) at every position and the same return class -- what the
    name-only checks cannot see: an argument dropped from a 23-parameter list shifts every later one."""
    import tfk_header
    from torchflows_amd import native
    protos = tfk_header.prototypes()
    assert len(protos) == 89 and list(protos) == list(native.SYMBOLS)          # the table follows the header's order
    for name, (ret, params) in protos.items():
        restype, argtypes = native._ABI[name]
        bound = [_ctype_class(t, native) for t in argtypes]
        assert len(bound) == len(params), f"{name}: {len(bound)} argtypes for {len(params)} parameters"
        for k, (b, (cls, pname)) in enumerate(zip(bound, params)):
            assert _same_class(b, cls), f"{name}: argument {k} ({pname}) is {cls} in the header, bound as {b}"
        assert _ctype_class(restype, native) == ret, f"{name}: returns {ret} in the header, restype says {restype}"


def test_structures_match_the_header():
    """The three ctypes structures: as many fields as their typedef struct, the same classes, the same order."""
    import tfk_header
    from torchflows_amd import native
    declared = tfk_header.structs()
    assert sorted(declared) == sorted(_STRUCTURES)
    for cname, pyname in _STRUCTURES.items():
        fields = getattr(native, pyname)._fields_
        assert [n for n, _ in fields] == [n for _, n, _ in declared[cname]], cname
        for (fname, ftype), (cls, _, count) in zip(fields, declared[cname]):
            if count is not None:
                assert issubclass(ftype, C.Array) and ftype._length_ == count, f"{cname}.{fname}"
                ftype = ftype._type_
            assert _ctype_class(ftype, native) == cls, f"{cname}.{fname}: {cls} in the header"


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "tfk.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(tfk_[a-z0-9_]+)\s*\(", text)))


def test_libtfk_exports_every_declared_symbol():
    from torchflows_amd import native
    L = C.CDLL(native.LIB_PATH)
    names = declared_symbols()
    assert len(names) >= 47 and set(names) == set(native.SYMBOLS)
    for n in names:
        assert hasattr(L, n), n
    L.tfk_abi_version.restype = C.c_int
    assert L.tfk_abi_version() == native.ABI_VERSION == 29


def test_cpu_restatement_exports_the_minimum_set(cpu_abi):
    assert cpu_abi.tfk_abi_version() == 29
    for n in ("tfk_affine_coupling_fwd", "tfk_affine_coupling_inv", "tfk_rqs_coupling_fwd", "tfk_rqs_coupling_inv",
              "tfk_elementwise_affine_fwd", "tfk_elementwise_affine_inv", "tfk_diag_gauss_logprob", "tfk_sum_f32",
              "tfk_permute", "tfk_shift_coupling_fwd", "tfk_shift_coupling_inv"):
        assert hasattr(cpu_abi, n), n
    # a stream on the host build is an error, reported through the ABI's own channel
    x = np.zeros((1, 2), np.float32)
    rc = cpu_abi.tfk_permute(ptr(x), None, ptr(np.zeros_like(x)), 1, 2, C.c_void_p(1))
    assert rc == 1 and b"stream" in cpu_abi.tfk_last_error()


@pytest.mark.parametrize("T", [2, 32, 128])
def test_affine_coupling_host_abi_vs_reference(cpu_abi, T):
    """x = [untouched half | target half]: tfk_affine_coupling_* with tgt_idx = NULL (HalfSplit tail) must give the
    reference's Affine.forward / inverse on the target half, leave the rest, and honour `accumulate`."""
    fx = load_golden("affine.npz")
    xb, h = fx[f"T{T}_x"], np.ascontiguousarray(fx[f"T{T}_h"])
    N, D = xb.shape[0], 2 * T
    x = np.ascontiguousarray(np.concatenate([np.full_like(xb, 7.0), xb], axis=1))
    for d, zk, lk in (("fwd", "z", "ld"), ("inv", "xinv", "ldinv")):
        z = np.empty_like(x)
        ld = np.full(N, 3.0, np.float32)
        rc = getattr(cpu_abi, f"tfk_affine_coupling_{d}")(ptr(x), ptr(h), ptr(z), ptr(ld), N, D, None, T, 1, None)
        assert rc == 0, cpu_abi.tfk_last_error()
        assert np.array_equal(z[:, :T], x[:, :T])
        assert rel(z[:, T:], fx[f"T{T}_{zk}"]) < 5e-6 and rel(ld - 3.0, fx[f"T{T}_{lk}"]) < 1e-5
    # an explicit index list (every other column) in place
    idx = np.arange(0, D, 2, dtype=np.int32)
    x2 = np.ascontiguousarray(np.zeros((N, D), np.float32))
    x2[:, idx] = xb
    ld = np.empty(N, np.float32)
    assert cpu_abi.tfk_affine_coupling_fwd(ptr(x2), ptr(h), ptr(x2), ptr(ld), N, D, ptr(idx), T, 0, None) == 0
    assert rel(x2[:, idx], fx[f"T{T}_z"]) < 5e-6 and np.all(x2[:, 1::2] == 0)


@pytest.mark.parametrize("tag", ["B50_K8", "B5_K8", "B50_K4"])
def test_rqs_coupling_host_abi_vs_reference(cpu_abi, tag):
    fx = load_golden("rqs.npz")
    xb, h = fx[f"{tag}_x"], np.ascontiguousarray(fx[f"{tag}_h"])
    N, T = xb.shape
    K = (h.shape[-1] + 1) // 3
    boundary = float(tag.split("_")[0][1:])
    x = np.ascontiguousarray(np.concatenate([np.zeros_like(xb), xb], axis=1))
    for d, zk, lk in (("fwd", "z", "ld"), ("inv", "xinv", "ldinv")):
        z, ld = np.empty_like(x), np.empty(N, np.float32)
        rc = getattr(cpu_abi, f"tfk_rqs_coupling_{d}")(ptr(x), ptr(h), ptr(z), ptr(ld), N, 2 * T, None, T, K,
                                                       _f(boundary), 0, None)
        assert rc == 0, cpu_abi.tfk_last_error()
        assert rel(z[:, T:], fx[f"{tag}_{zk}"]) < 4e-5 and rel(ld, fx[f"{tag}_{lk}"]) < 4e-5


def test_gauss_sum_permute_elementwise_host_abi(cpu_abi):
    fx = load_golden("gauss.npz")
    z = np.ascontiguousarray(fx["D64_value"])
    N, D = z.shape
    out = np.empty(N, np.float32)
    ldin = np.full(N, 2.0, np.float32)
    assert cpu_abi.tfk_diag_gauss_logprob(ptr(z), ptr(fx["D64_loc"]), ptr(fx["D64_log_scale"]), ptr(ldin), ptr(out),
                                          N, D, None) == 0
    assert rel(out - 2.0, fx["D64_log_prob"]) < 1e-5
    total = np.zeros(1, np.float64)
    assert cpu_abi.tfk_sum_f32(ptr(out), ptr(total), N, None) == 0
    assert abs(total[0] - out.astype(np.float64).sum()) < 1e-9 * abs(total[0])
    zr = np.empty_like(z)
    assert cpu_abi.tfk_permute(ptr(z), None, ptr(zr), N, D, None) == 0
    assert np.array_equal(zr, z[:, ::-1])
    # ElementwiseAffine / ActNorm with global parameters: fwd then inv is the identity, log-dets cancel
    rng = np.random.default_rng(0)
    value = np.ascontiguousarray(rng.standard_normal((D, 2)).astype(np.float32))
    for inverse_affine in (0, 1):
        y, ld = np.empty_like(z), np.empty(N, np.float32)
        assert cpu_abi.tfk_elementwise_affine_fwd(ptr(z), ptr(value), ptr(y), ptr(ld), N, D, inverse_affine, 0, None) == 0
        back = np.empty_like(z)
        assert cpu_abi.tfk_elementwise_affine_inv(ptr(y), ptr(value), ptr(back), ptr(ld), N, D, inverse_affine, 1, None) == 0
        assert rel(back, z) < 1e-5 and np.abs(ld).max() < 1e-4
