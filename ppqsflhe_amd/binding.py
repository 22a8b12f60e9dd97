"""ctypes binding of libmkckks_hip.so (C-ABI: include/mkckks.h).

Mirrors, for the hot path only, the OpenFHE CryptoContext calls the reference's
C++ mains make:
    cc->ReEncrypt(ct, reKey)          -> Context.reencrypt          changeCipherDomain.cpp:74
    cc->EvalAdd(ct1, ct2)             -> Context.eval_add           aggregateEncryptedWeights.cpp:82
    cc->EvalMult(ct, 0.5)             -> Context.rescale_mult_const aggregateEncryptedWeights.cpp:83
    cc->KeyGen() / ReKeyGen / Encrypt / Decrypt -> keygen / rekeygen / encrypt / decrypt
Buffers are DeviceBuffer objects (HBM, limb-major uint64) or anything with a
``data_ptr()`` (a torch tensor on the GPU).
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.environ.get("MKCKKS_LIB") or os.path.join(_HERE, "libmkckks_hip.so")  # override: A/B builds


class MkckksError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"mkckks error {code}: {msg}")
        self.code = code


class _Params(C.Structure):
    _fields_ = [("log_n", C.c_uint32), ("mult_depth", C.c_uint32), ("scaling_bits", C.c_uint32),
                ("first_bits", C.c_uint32), ("dnum", C.c_uint32), ("aux_bits", C.c_uint32),
                ("extra_bits", C.c_uint32), ("device", C.c_int32)]


class _Info(C.Structure):
    _fields_ = [("ring_dim", C.c_uint32), ("num_q", C.c_uint32), ("num_p", C.c_uint32),
                ("alpha", C.c_uint32), ("beta", C.c_uint32), ("slots", C.c_uint32)]


POLY_MAX_DEGREE, POLY_MAX_B = 63, 8  # MKCKKS_POLY_MAX_DEGREE, MKCKKS_POLY_MAX_B


class _PolyPlan(C.Structure):
    _fields_ = [("B", C.c_uint32), ("G", C.c_uint32), ("nl_T", C.c_uint32), ("nl_out", C.c_uint32),
                ("n_relin", C.c_uint32), ("depth", C.c_uint32), ("baby_nl", C.c_uint32 * (POLY_MAX_B - 1)),
                ("giant_nl", C.c_uint32 * (POLY_MAX_B - 1))]


# every symbol include/mkckks.h declares: name -> (restype, argtypes)
_vp, _u32, _u64p, _sz, _int, _dbl = C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t, C.c_int, C.c_double
SYMBOLS = {
    "mkckks_last_error": (C.c_char_p, []),
    "mkckks_version": (C.c_char_p, []),
    "mkckks_ctx_create": (_int, [C.POINTER(_Params), C.POINTER(_vp)]),
    "mkckks_ctx_destroy": (_int, [_vp]),
    "mkckks_ctx_info": (_int, [_vp, C.POINTER(_Info)]),
    "mkckks_ctx_moduli": (_int, [_vp, _u64p]),
    "mkckks_ctx_roots": (_int, [_vp, _u64p]),
    "mkckks_ctx_arith": (_int, [_vp, _vp]),
    "mkckks_scaling_factor": (_int, [_vp, _u32, _int, C.POINTER(_dbl)]),
    "mkckks_set_stream": (_int, [_vp, _vp]),
    "mkckks_sync": (_int, [_vp]),
    "mkckks_dev_alloc": (_int, [_vp, _sz, C.POINTER(_vp)]),
    "mkckks_dev_free": (_int, [_vp, _vp]),
    "mkckks_upload": (_int, [_vp, _vp, _vp, _sz]),
    "mkckks_download": (_int, [_vp, _vp, _vp, _sz]),
    "mkckks_host_alloc": (_int, [_vp, _sz, C.POINTER(_vp)]),
    "mkckks_host_free": (_int, [_vp, _vp]),
    "mkckks_upload_async": (_int, [_vp, _vp, _vp, _sz, C.POINTER(C.c_uint64)]),
    "mkckks_download_async": (_int, [_vp, _vp, _vp, _sz, C.POINTER(C.c_uint64)]),
    "mkckks_copy_done": (_int, [_vp, C.c_uint64, C.POINTER(_int)]),
    "mkckks_copy_wait": (_int, [_vp, C.c_uint64]),
    "mkckks_fence_uploads": (_int, [_vp]),
    "mkckks_fence_compute": (_int, [_vp]),
    "mkckks_count_noncanonical": (_int, [_vp, _vp, _u32, _u32, C.POINTER(C.c_uint64)]),
    "mkckks_debug_stamps": (_int, [_vp, _vp, _u32, C.POINTER(_sz)]),
    "mkckks_ntt_forward_batch": (_int, [_vp, _vp, _u32, _u32, _int]),
    "mkckks_ntt_inverse_batch": (_int, [_vp, _vp, _u32, _u32, _int]),
    "mkckks_eval_add_batch": (_int, [_vp, _vp, _vp, _vp, _u32, _u32]),
    "mkckks_eval_sum_batch": (_int, [_vp, _vp, _vp, _u32, _u32, _u32]),
    "mkckks_rescale_mult_const_batch": (_int, [_vp, _vp, _vp, _u32, _u32, _dbl]),
    "mkckks_rescale_batch": (_int, [_vp, _vp, _vp, _u32, _u32]),
    "mkckks_mult_const_batch": (_int, [_vp, _vp, _u32, _u32, _dbl]),
    "mkckks_mult_plain_batch": (_int, [_vp, _vp, _vp, _u32, _u32, _u32]),
    "mkckks_mult_plain_rescale_batch": (_int, [_vp, _vp, _vp, _vp, _u32, _u32, _u32]),
    "mkckks_reencrypt_batch": (_int, [_vp, _vp, _vp, _vp, _u32, _u32]),
    "mkckks_reencrypt_accumulate_batch": (_int, [_vp, _vp, _vp, _vp, _u32, _u32]),
    "mkckks_reencrypt_sum_batch": (_int, [_vp, _vp, _vp, _vp, _u32, _u32, _u32]),
    "mkckks_reencrypt_fanout_batch": (_int, [_vp, _vp, _vp, _vp, _u32, _u32, _u32]),
    "mkckks_scale_evk_batch": (_int, [_vp, _vp, _vp, _u32, _vp, _u32]),
    "mkckks_reencrypt_wsum_batch": (_int, [_vp, _vp, _vp, _vp, _u32, _u32, _u32, _vp, _u32]),
    "mkckks_eval_wsum_batch": (_int, [_vp, _vp, _vp, _u32, _u32, _u32, _vp, _u32, _int]),
    "mkckks_compress_batch": (_int, [_vp, _vp, _vp, _u32, _u32, _u32]),
    "mkckks_reencrypt_fanout_compact_batch": (_int, [_vp, _vp, _vp, _vp, _u32, _u32, _u32, _u32]),
    "mkckks_modup_batch": (_int, [_vp, _vp, _vp, _u32, _u32]),
    "mkckks_moddown_batch": (_int, [_vp, _vp, _vp, _u32, _u32]),
    "mkckks_keygen": (_int, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "mkckks_rekeygen": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mkckks_galois_element": (_int, [_vp, C.c_int32, C.POINTER(_u32)]),
    "mkckks_automorphism_batch": (_int, [_vp, _vp, _vp, _u32, _u32, _u32]),
    "mkckks_automorphism_secret": (_int, [_vp, _vp, _vp, _u32]),
    "mkckks_galois_keygen": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _u32, _vp]),
    "mkckks_rotate_batch": (_int, [_vp, _vp, _vp, _vp, _u32, _u32, _u32]),
    "mkckks_slot_sum_batch": (_int, [_vp, _vp, _vp, _vp, _u32, _u32, _u32]),
    "mkckks_encode_ext_batch": (_int, [_vp, _vp, _vp, _u32, _u32, _dbl]),
    "mkckks_linear_transform_batch": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _u32, _u32, _u32]),
    "mkckks_linear_transform_bsgs_batch": (_int, [_vp, _vp, _vp, _vp, _u32, _vp, _vp, _u32, _vp, _vp, _vp, _u32, _u32]),
    "mkckks_relin_keygen": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mkckks_tensor_sum_batch": (_int, [_vp, _vp, _vp, _vp, _u32, _u32, _u32]),
    "mkckks_relinearize_batch": (_int, [_vp, _vp, _vp, _vp, _u32, _u32]),
    "mkckks_mult_relin_batch": (_int, [_vp, _vp, _vp, _vp, _vp, _u32, _u32]),
    "mkckks_poly_plan": (_int, [_vp, _u32, _u32, _vp]),
    "mkckks_powers_batch": (_int, [_vp, _vp, _vp, _vp, _u32, _u32, _u32, _dbl, _vp, _vp]),
    "mkckks_poly_weights": (_int, [_vp, _vp, _u32, _u32, _dbl, _vp, C.POINTER(_dbl)]),
    "mkckks_poly_tensor_batch": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _u32, _u32, _u32]),
    "mkckks_poly_eval_batch": (_int, [_vp, _vp, _vp, _vp, _u32, _vp, _u32, _u32, _dbl, C.POINTER(_dbl)]),
    "mkckks_affine_batch": (_int, [_vp, _vp, _vp, _u32, _u32, _dbl, _dbl]),
    "mkckks_cheb_tensor_batch": (_int, [_vp, _vp, _u32, _vp, _u32, _vp, _u32, _dbl, _vp, _u32, _u32]),
    "mkckks_cheb_ladder_batch": (_int, [_vp, _vp, _vp, _vp, _u32, _u32, _u32, _dbl, _vp, _vp]),
    "mkckks_cheb_weights": (_int, [_vp, _vp, _u32, _u32, _dbl, _vp, C.POINTER(_dbl)]),
    "mkckks_cheb_eval_batch": (_int, [_vp, _vp, _vp, _vp, _u32, _dbl, _dbl, _vp, _u32, _u32, _dbl, C.POINTER(_dbl)]),
    "mkckks_evk_sum": (_int, [_vp, _vp, _vp, _u32, _u32]),
    "mkckks_relin_share": (_int, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "mkckks_keygen_join": (_int, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "mkckks_partial_decrypt_batch": (_int, [_vp, _vp, _vp, _vp, _vp, _u32, _u32, _u32, _int]),
    "mkckks_fuse_shares_batch": (_int, [_vp, _vp, _vp, _u32, _u32, _u32]),
    "mkckks_switch_share_batch": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _u32, _u32, _int]),
    "mkckks_share_key": (_int, [_vp, _vp, _vp, _u32, _u32, _u32, C.c_char_p, _u32]),
    "mkckks_combine_key_shares": (_int, [_vp, _vp, _vp, _vp, _u32, _u32]),
    "mkckks_lagrange_at_zero": (_int, [_vp, _vp, _u32, _vp]),
    "mkckks_q0_walk_choice": (_int, [_u32, _u32, _u32, _int]),
    "mkckks_icol_conv_targets": (_u32, [_u32, C.c_uint64, _int]),
    "mkckks_encrypt_batch": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _u32]),
    "mkckks_lift_ntt_batch": (_int, [_vp, _vp, _vp, _u32, _u32]),
    "mkckks_decrypt_batch": (_int, [_vp, _vp, _vp, _vp, _u32, _u32]),
    "mkckks_sample_ternary": (_int, [_vp, _vp, _sz, C.c_char_p, _u32]),
    "mkckks_sample_gauss": (_int, [_vp, _vp, _sz, _dbl, C.c_char_p, _u32]),
    "mkckks_sample_gauss_wide": (_int, [_vp, _vp, _sz, _dbl, C.c_char_p, _u32]),
    "mkckks_rerandomize_batch": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _u32, _u32]),
    "mkckks_sample_uniform": (_int, [_vp, _vp, _u32, _u32, _int, C.c_char_p, _u32]),
    "mkckks_chacha20_block": (_int, [_vp, _vp, C.c_char_p, _u32, C.POINTER(_u32)]),
    "mkckks_encrypt_seeded_batch": (_int, [_vp, _vp, _vp, _vp, _vp, _u32, _u32, C.c_char_p, _u32]),
    "mkckks_expand_seeded_batch": (_int, [_vp, _vp, _u32, _u32, C.c_char_p, C.POINTER(_u32)]),
    "mkckks_encode_batch": (_int, [_vp, _vp, _vp, _u32, _u32, _dbl]),
    "mkckks_decode_batch": (_int, [_vp, _vp, _vp, _u32, _u32, _dbl]),
    "mkckks_decode_flood_batch": (_int, [_vp, _vp, _vp, _u32, _u32, _dbl, C.c_char_p, _u32, _vp]),
    "mkckks_reduce_mod_batch": (_int, [_vp, _vp, _u32, _u32, _u32]),
    "mkckks_comm_unique_id": (_int, [_vp]),
    "mkckks_comm_create": (_int, [_vp, _vp, _int, _int, C.POINTER(_vp)]),
    "mkckks_comm_destroy": (_int, [_vp, _vp]),
    "mkckks_reduce_scatter_sum_mod": (_int, [_vp, _vp, _vp, _vp, _u32, _u32, _u32]),
    "mkckks_comm_library": (C.c_char_p, []),
    "mkckks_ctx_twiddles": (_int, [_vp, _u32, _int, _u64p]),
    "mkckks_debug_arith": (_int, [_vp, _u32, C.c_uint64, _vp, _vp, _sz]),
}
# ops of mkckks_debug_arith (MKCKKS_OP_* of include/mkckks.h): name -> (id, input planes, output planes, twiddle planes)
ARITH_OPS = {
    "csub": (0, 2, 1, 0),
    "add_mod": (1, 2, 1, 0),
    "sub_mod": (2, 2, 1, 0),
    "shoup_lazy": (3, 2, 1, 1),
    "shoup_mul": (4, 2, 1, 1),
    "mul_mod": (5, 2, 1, 0),
    "barrett_reduce128": (6, 2, 1, 0),
    "reduce_wide": (7, 2, 1, 0),
    "reduce_word": (8, 1, 1, 0),
    "reduce_cols_lazy": (9, 3, 1, 0),
    "reduce_cols": (10, 3, 1, 0),
    "reduce_cols4": (11, 4, 1, 0),
    "mac128": (12, 4, 2, 0),
    "mac128_split": (13, 4, 2, 0),
    "ct_butterfly_c4": (14, 3, 2, 1),
    "ct_butterfly_nc": (15, 3, 2, 1),
    "gs_butterfly": (16, 3, 2, 1),
    "canon8": (17, 1, 1, 0),
    "radix_forward4": (18, 31, 16, 15),
    "radix_inverse4": (19, 31, 16, 15),
    "pm_fold": (20, 1, 1, 0),
    "pm_lazy": (21, 2, 1, 1),
    "pm_reduce128": (22, 2, 1, 0),
    "pm_reduce_cols": (23, 3, 1, 0),
    "ct_butterfly_pm_f": (24, 3, 2, 1),
    "ct_butterfly_pm_n": (25, 3, 2, 1),
    "gs_butterfly_pm": (26, 3, 2, 1),
    "radix_forward_pm4": (27, 31, 16, 15),
    "radix_inverse_pm4": (28, 31, 16, 15),
    "fp_mulmod": (29, 2, 1, 1),
    "fp_reduce": (30, 1, 1, 0),
    "fp_to_canonical": (31, 1, 1, 0),
    "fp_mulmod_any": (32, 2, 1, 0),
    "u52_to_double": (33, 1, 1, 0),
    "split30_d": (34, 1, 2, 0),
    "ct_butterfly_fp": (35, 3, 2, 1),
    "ct_butterfly_fp_nr": (36, 3, 2, 1),
    "gs_butterfly_fp": (37, 3, 2, 1),
    "radix_forward_fp4": (38, 31, 16, 15),
    "radix_inverse_fp4": (39, 31, 16, 15),
}
COMM_ID_BYTES = 128
E_PRECISION = -6  # MKCKKS_E_PRECISION: decode_flood's noise estimate exceeds the context's precision

_lib = None


def lib_path():
    return _LIB


def hip_runtimes_loaded():
    """Distinct libamdhip64 files mapped into this process (more than one is the "no HIP device" trap)."""
    paths = []
    try:
        for line in open("/proc/self/maps"):
            if "libamdhip64" in line:
                p = line[line.index("/"):].strip()
                if p not in paths:
                    paths.append(p)
    except (OSError, ValueError):
        pass
    return paths


def load_library():
    """Load the in-tree HIP library; raise (never fall back) when it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB):
            raise ImportError(
                f"{_LIB} not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C ppqsflhe_amd/csrc` (hipcc --offload-arch=gfx950). There is no CPU fallback.")
        # PyTorch-ROCm ships its own libamdhip64: when both end up in one process the FIRST HIP runtime loaded owns
        # the device and the other reports "no ROCm-capable device".  Tensors from torch are this binding's device
        # buffers (bench.py, multi-GPU), so let torch load first whenever it is installed.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass  # no torch in this environment: the library's own runtime is the only one
        L = C.CDLL(_LIB)
        dup = hip_runtimes_loaded()
        if len(dup) > 1:
            import warnings
            warnings.warn("two HIP runtimes in this process (" + ", ".join(dup) + "): the one initialised second sees no "
                          "device; import torch before ppqsflhe_amd, or do not mix ROCm installations", RuntimeWarning)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def sampler_key(key):
    if isinstance(key, int):
        key = int(key).to_bytes(32, "little")
    key = bytes(key)
    if len(key) != 32:
        raise ValueError("sampler key must be 32 bytes")
    return key


def _ptr(x):
    if x is None:
        return None
    if isinstance(x, DeviceBuffer):
        return x.ptr
    if hasattr(x, "data_ptr"):  # torch tensor on the device
        return x.data_ptr()
    if isinstance(x, int):
        return x
    raise TypeError(f"expected a device buffer, got {type(x)}")


class DeviceBuffer:
    """A typed, shaped view of HBM owned by a Context."""

    def __init__(self, ctx, shape, dtype):
        self.ctx = ctx
        self.shape = tuple(int(s) for s in shape)
        self.dtype = np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize
        p = C.c_void_p()
        ctx._check(ctx._L.mkckks_dev_alloc(ctx._h, self.nbytes, C.byref(p)))
        self.ptr = p.value
        self._owned = True

    def upload(self, arr):
        arr = np.ascontiguousarray(arr, dtype=self.dtype)
        assert arr.nbytes == self.nbytes, (arr.shape, self.shape)
        self.ctx._check(self.ctx._L.mkckks_upload(self.ctx._h, self.ptr, arr.ctypes.data, self.nbytes))
        return self

    def to_host(self):
        out = np.empty(self.shape, dtype=self.dtype)
        self.ctx._check(self.ctx._L.mkckks_download(self.ctx._h, out.ctypes.data, self.ptr, self.nbytes))
        return out

    def view(self, offset_elems, shape):
        """A non-owning sub-view (element offset) of this buffer."""
        v = object.__new__(DeviceBuffer)
        v.ctx, v.shape, v.dtype = self.ctx, tuple(shape), self.dtype
        v.nbytes = int(np.prod(v.shape, dtype=np.int64)) * v.dtype.itemsize
        v.ptr = self.ptr + offset_elems * self.dtype.itemsize
        v._owned = False
        v._parent = self
        return v

    def free(self):
        if getattr(self, "_owned", False) and self.ptr and self.ctx._h:
            self.ctx._L.mkckks_dev_free(self.ctx._h, self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Context:
    """Device-resident CKKS context (moduli, twiddles, CRT tables in HBM)."""

    def __init__(self, log_n, mult_depth, scaling_bits, first_bits=60, dnum=3, aux_bits=60, extra_bits=20,
                 device=0):
        self._L = load_library()
        self._h = None
        p = _Params(log_n, mult_depth, scaling_bits, first_bits, dnum, aux_bits, extra_bits, device)
        h = C.c_void_p()
        self._check(self._L.mkckks_ctx_create(C.byref(p), C.byref(h)))
        self._h = h.value
        info = _Info()
        self._check(self._L.mkckks_ctx_info(self._h, C.byref(info)))
        self.N, self.L, self.K = info.ring_dim, info.num_q, info.num_p
        self.D = self.L + self.K
        self.alpha, self.beta, self.slots = info.alpha, info.beta, info.slots
        self.device = device
        self.moduli = np.zeros(self.D, dtype=np.uint64)
        self.roots = np.zeros(self.D, dtype=np.uint64)
        self._check(self._L.mkckks_ctx_moduli(self._h, self.moduli.ctypes.data))
        self._check(self._L.mkckks_ctx_roots(self._h, self.roots.ctypes.data))
        # arithmetic class of every limb on the device: 0 integer (Shoup), 1 fp64, 2 integer (pseudo-Mersenne)
        self.arith = np.zeros(self.D, dtype=np.uint8)
        self._check(self._L.mkckks_ctx_arith(self._h, self.arith.ctypes.data))

    def _check(self, rc):
        if rc != 0:
            raise MkckksError(rc, self._L.mkckks_last_error().decode())

    def close(self):
        if self._h:
            for p in list(getattr(self, "_pinned", {}).values()):  # pinned buffers the caller did not give back
                self._L.mkckks_host_free(self._h, p)
            self._pinned = {}
            self._L.mkckks_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- parameters
    def sf(self, level):
        out = C.c_double()
        self._check(self._L.mkckks_scaling_factor(self._h, level, 0, C.byref(out)))
        return out.value

    def sf_big(self, level):
        out = C.c_double()
        self._check(self._L.mkckks_scaling_factor(self._h, level, 1, C.byref(out)))
        return out.value

    def twiddles(self, limb, inverse=False):
        out = np.zeros(self.N, dtype=np.uint64)
        self._check(self._L.mkckks_ctx_twiddles(self._h, limb, int(inverse), out.ctypes.data))
        return out

    def debug_arith(self, op, q, operands):
        """Diagnostics: run primitive `op` (a name of ARITH_OPS) once per element of the operand planes
        uint64[n_in][count] under modulus q; returns uint64[n_out][count].  Device context: the device form, on the
        stream; device=-1: the host form.  Doubles travel as bit patterns; twiddle planes hold w only."""
        opid, n_in, n_out, _ = ARITH_OPS[op]
        x = np.ascontiguousarray(operands, dtype=np.uint64)
        assert x.ndim == 2 and x.shape[0] == n_in, (op, x.shape)
        count = x.shape[1]
        if self.device < 0:
            out = np.zeros((n_out, count), dtype=np.uint64)
            self._check(self._L.mkckks_debug_arith(self._h, opid, int(q), x.ctypes.data, out.ctypes.data, count))
            return out
        if count == 0:
            self._check(self._L.mkckks_debug_arith(self._h, opid, int(q), None, None, 0))
            return np.zeros((n_out, 0), dtype=np.uint64)
        d_in, d_out = self.to_device(x), self.empty((n_out, count))
        try:
            self._check(self._L.mkckks_debug_arith(self._h, opid, int(q), d_in.ptr, d_out.ptr, count))
            return d_out.to_host()
        finally:
            d_in.free()
            d_out.free()

    def num_parts(self, nl):
        return min(self.beta, -(-nl // self.alpha))

    # ---- memory / stream
    def empty(self, shape, dtype=np.uint64):
        return DeviceBuffer(self, shape, dtype)

    def to_device(self, arr, dtype=None):
        arr = np.ascontiguousarray(arr, dtype=dtype or arr.dtype)
        return DeviceBuffer(self, arr.shape, arr.dtype).upload(arr)

    def set_stream(self, stream_handle):
        self._check(self._L.mkckks_set_stream(self._h, stream_handle))

    def sync(self):
        self._check(self._L.mkckks_sync(self._h))

    # ---- transforms (in place)
    def ntt_forward(self, d_polys, n_polys, nl, with_p=False):
        self._check(self._L.mkckks_ntt_forward_batch(self._h, _ptr(d_polys), n_polys, nl, int(with_p)))

    def ntt_inverse(self, d_polys, n_polys, nl, with_p=False):
        self._check(self._L.mkckks_ntt_inverse_batch(self._h, _ptr(d_polys), n_polys, nl, int(with_p)))

    # ---- aggregation
    def eval_add(self, a, b, out, n_ct, nl):
        self._check(self._L.mkckks_eval_add_batch(self._h, _ptr(a), _ptr(b), _ptr(out), n_ct, nl))

    def eval_sum(self, inp, out, n_clients, n_ct, nl):
        self._check(self._L.mkckks_eval_sum_batch(self._h, _ptr(inp), _ptr(out), n_clients, n_ct, nl))

    def rescale_mult_const(self, inp, out, n_ct, nl, operand):
        self._check(self._L.mkckks_rescale_mult_const_batch(self._h, _ptr(inp), _ptr(out), n_ct, nl, float(operand)))

    def rescale(self, inp, out, n_ct, nl):
        self._check(self._L.mkckks_rescale_batch(self._h, _ptr(inp), _ptr(out), n_ct, nl))

    def mult_const(self, ct, n_ct, nl, operand):
        self._check(self._L.mkckks_mult_const_batch(self._h, _ptr(ct), n_ct, nl, float(operand)))

    def mult_plain(self, ct, pt, n_ct, n_pt, nl):
        """EvalMult(ct, plaintext) core in place: ct[b] *= pt[b % n_pt]; pt as encode() writes it, n_pt is n_ct or 1."""
        self._check(self._L.mkckks_mult_plain_batch(self._h, _ptr(ct), _ptr(pt), n_ct, n_pt, nl))

    def mult_plain_rescale(self, inp, pt, out, n_ct, n_pt, nl):
        """out[n_ct][2][nl-1][N] = Rescale(inp * pt); inp is not modified and must not overlap out."""
        self._check(self._L.mkckks_mult_plain_rescale_batch(self._h, _ptr(inp), _ptr(pt), _ptr(out), n_ct, n_pt, nl))

    def reduce_mod(self, ct, n_ct, nl, n_terms):
        self._check(self._L.mkckks_reduce_mod_batch(self._h, _ptr(ct), n_ct, nl, n_terms))

    # ---- I/O pipeline (pinned host buffers, asynchronous copies with tickets, fences; include/mkckks.h)
    def host_alloc(self, nbytes):
        """Pinned host buffer as a numpy uint8 array (free it with host_free(array))."""
        p = C.c_void_p()
        self._check(self._L.mkckks_host_alloc(self._h, nbytes, C.byref(p)))
        arr = np.ctypeslib.as_array((C.c_uint8 * nbytes).from_address(p.value))
        self._pinned = getattr(self, "_pinned", {})
        self._pinned[arr.ctypes.data] = p.value
        return arr

    def host_free(self, arr):
        self._check(self._L.mkckks_host_free(self._h, self._pinned.pop(arr.ctypes.data)))

    def upload_async(self, dev, host_arr, nbytes=None):
        t = C.c_uint64()
        self._check(self._L.mkckks_upload_async(self._h, _ptr(dev), host_arr.ctypes.data,
                                                host_arr.nbytes if nbytes is None else nbytes, C.byref(t)))
        return t.value

    def download_async(self, host_arr, dev, nbytes=None):
        t = C.c_uint64()
        self._check(self._L.mkckks_download_async(self._h, host_arr.ctypes.data, _ptr(dev),
                                                  host_arr.nbytes if nbytes is None else nbytes, C.byref(t)))
        return t.value

    def copy_done(self, ticket):
        d = C.c_int()
        self._check(self._L.mkckks_copy_done(self._h, ticket, C.byref(d)))
        return bool(d.value)

    def copy_wait(self, ticket):
        self._check(self._L.mkckks_copy_wait(self._h, ticket))

    def fence_uploads(self):
        self._check(self._L.mkckks_fence_uploads(self._h))

    def fence_compute(self):
        self._check(self._L.mkckks_fence_compute(self._h))

    def count_noncanonical(self, ct, n_ct, nl):
        c = C.c_uint64()
        self._check(self._L.mkckks_count_noncanonical(self._h, _ptr(ct), n_ct, nl, C.byref(c)))
        return c.value

    # ---- RCCL exchange of the per-GPU partial sums (behind the C-ABI; librccl resolved by the library)
    def comm_unique_id(self):
        """Rank 0: the MKCKKS_COMM_ID_BYTES bootstrap bytes (ncclGetUniqueId) to hand to every other rank."""
        buf = C.create_string_buffer(COMM_ID_BYTES)
        self._check(self._L.mkckks_comm_unique_id(buf))
        return buf.raw

    def comm_create(self, unique_id, n_ranks, rank):
        """Collective: an ncclComm_t (opaque handle) for this context's device."""
        if len(unique_id) != COMM_ID_BYTES:
            raise ValueError("communicator id must be MKCKKS_COMM_ID_BYTES long")
        h = C.c_void_p()
        self._check(self._L.mkckks_comm_create(self._h, C.c_char_p(unique_id), n_ranks, rank, C.byref(h)))
        return h.value

    def comm_destroy(self, comm):
        self._check(self._L.mkckks_comm_destroy(self._h, comm))

    def reduce_scatter_sum_mod(self, comm, partial, shard, n_ct_shard, nl, n_ranks):
        self._check(self._L.mkckks_reduce_scatter_sum_mod(self._h, comm, _ptr(partial), _ptr(shard), n_ct_shard, nl,
                                                          n_ranks))

    def comm_library(self):
        return self._L.mkckks_comm_library().decode()

    # ---- proxy re-encryption
    def reencrypt(self, ct, evk, out, n_ct, nl):
        self._check(self._L.mkckks_reencrypt_batch(self._h, _ptr(ct), _ptr(evk), _ptr(out), n_ct, nl))

    def reencrypt_accumulate(self, ct, evk, acc, n_ct, nl):
        self._check(self._L.mkckks_reencrypt_accumulate_batch(self._h, _ptr(ct), _ptr(evk), _ptr(acc), n_ct, nl))

    def reencrypt_sum(self, cts, evks, out, n_clients, n_ct, nl):
        self._check(self._L.mkckks_reencrypt_sum_batch(self._h, _ptr(cts), _ptr(evks), _ptr(out), n_clients, n_ct, nl))

    # weighted aggregation: weights are host doubles, M_k = trunc(w_k * sf(sf_level) + 0.5) (include/mkckks.h)
    def scale_evk(self, evks, out, n_keys, weights, sf_level):
        w = np.ascontiguousarray(weights, dtype=np.float64)
        assert w.size == n_keys
        self._check(self._L.mkckks_scale_evk_batch(self._h, _ptr(evks), _ptr(out), n_keys, w.ctypes.data, sf_level))

    def reencrypt_wsum(self, cts, evks_scaled, out, n_clients, n_ct, nl, weights, sf_level):
        w = np.ascontiguousarray(weights, dtype=np.float64)
        assert w.size == n_clients
        self._check(self._L.mkckks_reencrypt_wsum_batch(self._h, _ptr(cts), _ptr(evks_scaled), _ptr(out), n_clients, n_ct, nl,
                                                        w.ctypes.data, sf_level))

    def eval_wsum(self, inp, out, n_terms, n_ct, nl, weights, sf_level, first_is_sum=False):
        w = np.ascontiguousarray(weights, dtype=np.float64)
        assert w.size == n_terms
        self._check(self._L.mkckks_eval_wsum_batch(self._h, _ptr(inp), _ptr(out), n_terms, n_ct, nl, w.ctypes.data, sf_level,
                                                   int(first_is_sum)))

    def reencrypt_fanout(self, ct, evks, out, n_keys, n_ct, nl):
        """out[k][b] = ReEncrypt(ct[b], evks[k]): one ciphertext batch into n_keys key domains (ModUp shared)."""
        self._check(self._L.mkckks_reencrypt_fanout_batch(self._h, _ptr(ct), _ptr(evks), _ptr(out), n_keys, n_ct, nl))

    def rerandomize(self, ct, pk, v, e0, e1, out, n_ct, nl_in, nl):
        """out[t] = first nl limbs of ct[t] + Enc_pk(0; v[t], e0[t], e1[t]): the re-randomisation of the HRA-secure
        ReEncrypt(ct, evk, pk); follow with any reencrypt* call.  v int8, e0 / e1 int64 (sample_gauss_wide)."""
        self._check(self._L.mkckks_rerandomize_batch(self._h, _ptr(ct), _ptr(pk), _ptr(v), _ptr(e0), _ptr(e1), _ptr(out),
                                                     n_ct, nl_in, nl))

    def compress(self, inp, out, n_ct, nl_in, nl_out):
        """out[b] = Rescale(first nl_out + 1 limbs of inp[b]): a ciphertext that will only be decrypted, at nl_out limbs."""
        self._check(self._L.mkckks_compress_batch(self._h, _ptr(inp), _ptr(out), n_ct, nl_in, nl_out))

    def reencrypt_fanout_compact(self, ct, evks, out, n_keys, n_ct, nl_in, nl_out):
        """out[k][b] = Rescale(ReEncrypt(first nl_out + 1 limbs of ct[b], evks[k])): the fan-out written at nl_out limbs."""
        self._check(self._L.mkckks_reencrypt_fanout_compact_batch(self._h, _ptr(ct), _ptr(evks), _ptr(out), n_keys, n_ct,
                                                                  nl_in, nl_out))

    def modup(self, c1, digits, n, nl):
        self._check(self._L.mkckks_modup_batch(self._h, _ptr(c1), _ptr(digits), n, nl))

    def moddown(self, inp, out, n, nl):
        self._check(self._L.mkckks_moddown_batch(self._h, _ptr(inp), _ptr(out), n, nl))

    # ---- keys and client endpoints
    def keygen(self, s, a, e, pk, sk):
        self._check(self._L.mkckks_keygen(self._h, _ptr(s), _ptr(a), _ptr(e), _ptr(pk), _ptr(sk)))

    def keygen_join(self, pk_prev, s, e, pk, sk):
        """MultipartyKeyGen(prevPublicKey): pk = (pk_prev[0] + e - pk_prev[1] * s, pk_prev[1]); the last party's pk is the
        joint key, whose secret is the sum of the parties' sk."""
        self._check(self._L.mkckks_keygen_join(self._h, _ptr(pk_prev), _ptr(s), _ptr(e), _ptr(pk), _ptr(sk)))

    def rekeygen(self, s_old, pk_new, u, e0, e1, evk):
        self._check(self._L.mkckks_rekeygen(self._h, _ptr(s_old), _ptr(pk_new), _ptr(u), _ptr(e0), _ptr(e1), _ptr(evk)))

    # ---- slot rotations (include/mkckks.h: "slot rotations and slot sums")
    def galois_element(self, step):
        """5^step mod 2N: the element that rotates the slots left by `step` (negative: right).  Host only."""
        g = C.c_uint32()
        self._check(self._L.mkckks_galois_element(self._h, int(step), C.byref(g)))
        return g.value

    @property
    def galois_conj(self):
        """MKCKKS_GALOIS_CONJ: 2N - 1, the element of the complex conjugation."""
        return 2 * self.N - 1

    def automorphism(self, inp, out, n_polys, nl, g):
        self._check(self._L.mkckks_automorphism_batch(self._h, _ptr(inp), _ptr(out), n_polys, nl, g))

    def automorphism_secret(self, s, out, g):
        self._check(self._L.mkckks_automorphism_secret(self._h, _ptr(s), _ptr(out), g))

    def galois_keygen(self, s, pk, u, e0, e1, g, evk):
        """The Galois key for g: rekeygen(sigma_g(s), pk, u, e0, e1)."""
        self._check(self._L.mkckks_galois_keygen(self._h, _ptr(s), _ptr(pk), _ptr(u), _ptr(e0), _ptr(e1), g, _ptr(evk)))

    def rotate(self, ct, evk, out, n_ct, nl, g):
        self._check(self._L.mkckks_rotate_batch(self._h, _ptr(ct), _ptr(evk), _ptr(out), n_ct, nl, g))

    def slot_sum(self, ct, evks, out, n_ct, nl, span):
        """out = ct + its rotations by 1 .. span - 1; evks [log2 span][beta][2][D][N], key k for step 2^k."""
        self._check(self._L.mkckks_slot_sum_batch(self._h, _ptr(ct), _ptr(evks), _ptr(out), n_ct, nl, span))

    # ---- linear transforms (include/mkckks.h: "linear transforms by diagonals, double hoisted")
    def encode_ext(self, vals, pt, n, nl, scale):
        """encode over the extended basis: pt u64[n][nl+K][N], Q limbs (those of encode) then P limbs."""
        self._check(self._L.mkckks_encode_ext_batch(self._h, _ptr(vals), _ptr(pt), n, nl, float(scale)))

    def linear_transform(self, ct, evks, pts, gs, out, n_ct, nl):
        """out[b] = sum_r pts[r] * Rotate(ct[b], gs[r]) before the rescale, double hoisted: evks [n_rot][beta][2][D][N],
        pts [n_rot][nl+K][N] from encode_ext, gs the n_rot Galois elements (host integers; 1: no rotation, no key)."""
        gs = [int(g) for g in gs]
        arr = (C.c_uint32 * max(1, len(gs)))(*gs)
        self._check(self._L.mkckks_linear_transform_batch(self._h, _ptr(ct), _ptr(evks), _ptr(pts), arr, _ptr(out), len(gs),
                                                          n_ct, nl))

    def linear_transform_bsgs(self, ct, bkeys, gb, gkeys, gg, pts, present, out, n_ct, nl):
        """The baby-step giant-step form: out[b] = sum_t Rotate(sum_b pts[t][b] * Rotate(ct[b], gb[b]), gg[t]) before the
        rescale.  bkeys [n1][beta][2][D][N] and gkeys [n2][..] (None when every element of the list is 1), gb / gg the
        Galois elements (host integers), pts [n2][n1][nl+K][N] from encode_ext, present: n2 x n1 host flags."""
        gb, gg = [int(g) for g in gb], [int(g) for g in gg]
        flags = [1 if f else 0 for row in present for f in row]
        a_gb, a_gg = (C.c_uint32 * max(1, len(gb)))(*gb), (C.c_uint32 * max(1, len(gg)))(*gg)
        a_pr = (C.c_uint8 * max(1, len(flags)))(*flags)
        if len(flags) != len(gb) * len(gg):
            raise ValueError("present must be n2 rows of n1 flags")
        self._check(self._L.mkckks_linear_transform_bsgs_batch(self._h, _ptr(ct), _ptr(bkeys), a_gb, len(gb), _ptr(gkeys),
                                                               a_gg, len(gg), _ptr(pts), a_pr, _ptr(out), n_ct, nl))

    # ---- ciphertext products (include/mkckks.h: "ciphertext products")
    def relin_keygen(self, s, pk, u, e0, e1, evk):
        """The relinearisation key of s: rekeygen with NTT(s_old) replaced by NTT(s)^2."""
        self._check(self._L.mkckks_relin_keygen(self._h, _ptr(s), _ptr(pk), _ptr(u), _ptr(e0), _ptr(e1), _ptr(evk)))

    def tensor_sum(self, a, b, out3, n_terms, n_ct, nl):
        """out3[b] = sum_t (a0 b0, a0 b1 + a1 b0, a1 b1); a, b [n_terms][n_ct][2][nl][N], out3 [n_ct][3][nl][N]."""
        self._check(self._L.mkckks_tensor_sum_batch(self._h, _ptr(a), _ptr(b), _ptr(out3), n_terms, n_ct, nl))

    def relinearize(self, in3, rlk, out, n_ct, nl):
        """out = (d0, d1) + KeySwitch(d2, rlk)."""
        self._check(self._L.mkckks_relinearize_batch(self._h, _ptr(in3), _ptr(rlk), _ptr(out), n_ct, nl))

    def mult_relin(self, a, b, rlk, out, n_ct, nl):
        """out = Relinearize(a x b); out may be a or b; a is b squares."""
        self._check(self._L.mkckks_mult_relin_batch(self._h, _ptr(a), _ptr(b), _ptr(rlk), _ptr(out), n_ct, nl))

    # ---- polynomial evaluation (include/mkckks.h: "polynomial evaluation")
    def poly_plan(self, degree, nl):
        """The plan of a degree-`degree` evaluation from nl limbs: dict(B, G, nl_T, nl_out, n_relin, depth, baby_nl [B-1],
        giant_nl [G-1]).  Host only."""
        p = _PolyPlan()
        self._check(self._L.mkckks_poly_plan(self._h, int(degree), int(nl), C.byref(p)))
        return dict(B=p.B, G=p.G, nl_T=p.nl_T, nl_out=p.nl_out, n_relin=p.n_relin, depth=p.depth,
                    baby_nl=list(p.baby_nl[:p.B - 1]), giant_nl=list(p.giant_nl[:p.G - 1]))

    def powers(self, z, rlk, out, n_ct, nl, n_pow, scale_in):
        """out = z^1 .. z^n_pow, power k packed [n_ct][2][nl_k][N] behind power k - 1; returns (nl_k list, S_k list)."""
        n_pow = int(n_pow)
        if not 1 <= n_pow <= 64:
            raise ValueError("n_pow must be in [1, 64]")
        nls, scales = (C.c_uint32 * n_pow)(), (C.c_double * n_pow)()
        self._check(self._L.mkckks_powers_batch(self._h, _ptr(z), _ptr(rlk), _ptr(out), n_ct, nl, n_pow, float(scale_in),
                                                C.addressof(nls), C.addressof(scales)))
        return list(nls), list(scales)

    def poly_weights(self, coef, nl, scale_in):
        """(w float64[G][B], S_out) of the polynomial with the power-basis coefficients coef[0 .. d] from nl limbs.  Host only."""
        c = np.ascontiguousarray(coef, dtype=np.float64)
        if c.ndim != 1 or not 3 <= c.size <= POLY_MAX_DEGREE + 1:
            raise ValueError("coef must hold the 3 .. 64 coefficients of a polynomial of degree 2 .. 63")
        plan = self.poly_plan(c.size - 1, nl)
        w = np.zeros((plan["G"], plan["B"]), dtype=np.float64)
        s_out = C.c_double()
        self._check(self._L.mkckks_poly_weights(self._h, c.ctypes.data, c.size - 1, int(nl), float(scale_in), w.ctypes.data,
                                                C.byref(s_out)))
        return w, s_out.value

    def poly_tensor(self, baby, baby_nl, giant, giant_nl, w, out3, n_ct, nl_T):
        """out3 [n_ct][3][nl_T][N] = the fused outer sum over babies x^1 .. x^{B-1} and giants y^1 .. y^{G-1} (each packed
        like the output of powers, limb counts baby_nl / giant_nl) with the weights w float64[G][B]."""
        w = np.ascontiguousarray(w, dtype=np.float64)
        if w.ndim != 2:
            raise ValueError("w must be float64[G][B]")
        G, B = w.shape
        if len(baby_nl) != B - 1 or len(giant_nl) != G - 1:
            raise ValueError("baby_nl needs B - 1 entries and giant_nl G - 1")
        bn = (C.c_uint32 * max(1, B - 1))(*[int(v) for v in baby_nl])
        gn = (C.c_uint32 * max(1, G - 1))(*[int(v) for v in giant_nl])
        self._check(self._L.mkckks_poly_tensor_batch(self._h, _ptr(baby), C.addressof(bn), _ptr(giant), C.addressof(gn),
                                                     w.ctypes.data, _ptr(out3), B, G, n_ct, nl_T))

    def poly_eval(self, ct, rlk, coef, out, n_ct, nl, scale_in):
        """out [n_ct][2][nl_out][N] = p(ct) slot-wise for the power-basis coefficients coef[0 .. d]; returns S_out."""
        c = np.ascontiguousarray(coef, dtype=np.float64)
        if c.ndim != 1 or not 3 <= c.size <= POLY_MAX_DEGREE + 1:
            raise ValueError("coef must hold the 3 .. 64 coefficients of a polynomial of degree 2 .. 63")
        s_out = C.c_double()
        self._check(self._L.mkckks_poly_eval_batch(self._h, _ptr(ct), _ptr(rlk), c.ctypes.data, c.size - 1, _ptr(out), n_ct,
                                                   int(nl), float(scale_in), C.byref(s_out)))
        return s_out.value

    # ---- Chebyshev series (include/mkckks.h: "Chebyshev series")
    def affine(self, inp, out, n_ct, nl, w_mul, w_add):
        """out = rint(w_mul) * inp + (rint(w_add), 0) as exact integers mod q_t; no rescale; out may be inp."""
        self._check(self._L.mkckks_affine_batch(self._h, _ptr(inp), _ptr(out), n_ct, int(nl), float(w_mul), float(w_add)))

    def cheb_tensor(self, a, nl_a, b, nl_b, t, nl_t, w, out3, n_ct, nl):
        """out3 [n_ct][3][nl][N] = (2 a0 b0 - M t0, 2 (a0 b1 + a1 b0) - M t1, 2 a1 b1), M = rint(w); a, b, t read in place at
        nl_a, nl_b, nl_t limbs; t None is the constant 1; a is b squares."""
        self._check(self._L.mkckks_cheb_tensor_batch(self._h, _ptr(a), int(nl_a), _ptr(b), int(nl_b), _ptr(t), int(nl_t),
                                                     float(w), _ptr(out3), n_ct, int(nl)))

    def cheb_ladder(self, u, rlk, out, n_ct, nl, n, scale_in):
        """out = T_1(u) .. T_n(u), T_k packed [n_ct][2][nl_k][N] behind T_{k-1}; returns (nl_k list, S_k list)."""
        n = int(n)
        if not 1 <= n <= 64:
            raise ValueError("n must be in [1, 64]")
        nls, scales = (C.c_uint32 * n)(), (C.c_double * n)()
        self._check(self._L.mkckks_cheb_ladder_batch(self._h, _ptr(u), _ptr(rlk), _ptr(out), n_ct, int(nl), n, float(scale_in),
                                                     C.addressof(nls), C.addressof(scales)))
        return list(nls), list(scales)

    def cheb_weights(self, coef, nl, scale_in):
        """(w float64[G][B], S_out) of the series sum_k coef[k] T_k(u) for u at nl limbs and scale scale_in.  Host only."""
        c = np.ascontiguousarray(coef, dtype=np.float64)
        if c.ndim != 1 or not 3 <= c.size <= POLY_MAX_DEGREE + 1:
            raise ValueError("coef must hold the 3 .. 64 coefficients of a series of degree 2 .. 63")
        plan = self.poly_plan(c.size - 1, nl)
        w = np.zeros((plan["G"], plan["B"]), dtype=np.float64)
        s_out = C.c_double()
        self._check(self._L.mkckks_cheb_weights(self._h, c.ctypes.data, c.size - 1, int(nl), float(scale_in), w.ctypes.data,
                                                C.byref(s_out)))
        return w, s_out.value

    def cheb_eval(self, ct, rlk, coef, a, b, out, n_ct, nl, scale_in):
        """out [n_ct][2][nl_out][N] = sum_k coef[k] T_k(u) slot-wise, u = the map of [a, b] onto [-1, 1]; returns S_out."""
        c = np.ascontiguousarray(coef, dtype=np.float64)
        if c.ndim != 1 or not 2 <= c.size <= POLY_MAX_DEGREE + 2:  # degrees 1 and 64 reach the library, which refuses them
            raise ValueError("coef must hold the coefficients of a series of degree 2 .. 63")
        s_out = C.c_double()
        self._check(self._L.mkckks_cheb_eval_batch(self._h, _ptr(ct), _ptr(rlk), c.ctypes.data, c.size - 1, float(a), float(b),
                                                   _ptr(out), n_ct, int(nl), float(scale_in), C.byref(s_out)))
        return s_out.value

    # ---- collective evaluation keys of a joint key (include/mkckks.h: "collective evaluation keys")
    def evk_sum(self, shares, out, n_parties, n_keys):
        """out[k] = sum_p shares[p][k] on all D limbs; shares [n_parties][n_keys][beta][2][D][N]; out may be shares[0]."""
        self._check(self._L.mkckks_evk_sum(self._h, _ptr(shares), _ptr(out), n_parties, n_keys))

    def relin_share(self, key1, sk, e0, e1, share):
        """Round 2 of the collective relinearisation key: share = key1 * sk + NTT(e) on all D limbs; share may be key1."""
        self._check(self._L.mkckks_relin_share(self._h, _ptr(key1), _ptr(sk), _ptr(e0), _ptr(e1), _ptr(share)))

    def encrypt(self, pk, pt, v, e0, e1, ct, n_ct, nl):
        self._check(self._L.mkckks_encrypt_batch(self._h, _ptr(pk), _ptr(pt), _ptr(v), _ptr(e0), _ptr(e1), _ptr(ct),
                                                 n_ct, nl))

    def encrypt_seeded(self, sk, pt, e, c0, n_ct, nl, seed, stream_base=0):
        """cc->Encrypt(privateKey, pt) with a seeded a (include/mkckks.h: mkckks_encrypt_seeded_batch): item t's a is
        sample_uniform(1, nl, 0, seed, stream_base + t); writes c0 u64[n_ct][nl][N] only."""
        self._check(self._L.mkckks_encrypt_seeded_batch(self._h, _ptr(sk), _ptr(pt), _ptr(e), _ptr(c0), n_ct, nl,
                                                        sampler_key(seed), stream_base))

    def expand_seeded(self, ct, n_ct, nl, seeds, stream_ids):
        """rebuild c1 of seeded ciphertexts in place (mkckks_expand_seeded_batch): ct u64[n_ct][2][nl][N]; `seeds`: n_ct
        32-byte keys (bytes, or ints as for the samplers), `stream_ids`: n_ct stream ids."""
        keys = b"".join(sampler_key(k) for k in seeds)
        sids = np.ascontiguousarray(stream_ids, dtype=np.uint32)
        if len(keys) != 32 * n_ct or sids.size != n_ct:
            raise ValueError("expand_seeded: need one seed and one stream id per ciphertext")
        self._check(self._L.mkckks_expand_seeded_batch(self._h, _ptr(ct), n_ct, nl, keys,
                                                       sids.ctypes.data_as(C.POINTER(_u32))))

    def lift_ntt(self, coef, out, n, nl):
        self._check(self._L.mkckks_lift_ntt_batch(self._h, _ptr(coef), _ptr(out), n, nl))

    # ---- samplers: `key` is the 32-byte ChaCha20 key (bytes); an int is accepted for tests and expanded
    # little-endian with zero padding (a test vector, NOT a way to key production randomness)
    def sample_ternary(self, out, count, key, stream_id=0):
        self._check(self._L.mkckks_sample_ternary(self._h, _ptr(out), count, sampler_key(key), stream_id))

    def sample_gauss(self, out, count, sigma, key, stream_id=0):
        self._check(self._L.mkckks_sample_gauss(self._h, _ptr(out), count, float(sigma), sampler_key(key), stream_id))

    def sample_gauss_wide(self, out, count, sigma, key, stream_id=0):
        """int64 rint(sigma * z), z standard normal (mkckks_sample_gauss_wide): the errors of `rerandomize`."""
        self._check(self._L.mkckks_sample_gauss_wide(self._h, _ptr(out), count, float(sigma), sampler_key(key), stream_id))

    def sample_uniform(self, out, n_polys, nl, with_p, key, stream_id=0):
        self._check(self._L.mkckks_sample_uniform(self._h, _ptr(out), n_polys, nl, int(with_p), sampler_key(key), stream_id))

    def chacha20_block(self, key, counter, nonce):
        out = self.empty((16,), np.uint32)
        n3 = (C.c_uint32 * 3)(*nonce)
        self._check(self._L.mkckks_chacha20_block(self._h, out.ptr, sampler_key(key), counter, n3))
        return out.to_host()

    def encode(self, vals, pt, n, nl, scale):
        self._check(self._L.mkckks_encode_batch(self._h, _ptr(vals), _ptr(pt), n, nl, float(scale)))

    def decode(self, m, vals, n, nl, scale):
        self._check(self._L.mkckks_decode_batch(self._h, _ptr(m), _ptr(vals), n, nl, float(scale)))

    def decode_flood(self, m, vals, n, nl, scale, key, stream_id=0):
        """decode with upstream Decode's noise estimate + flooding (include/mkckks.h: mkckks_decode_flood_batch);
        `key`: the 32-byte ChaCha20 key of the flooding normals.  Returns log2 sigma_hat per item (float64[n]).  An
        item over the precision limit raises MkckksError with code E_PRECISION after every output was written; the
        array is then on the exception as `log2_sigma`."""
        log2 = np.zeros(n, dtype=np.float64)
        rc = self._L.mkckks_decode_flood_batch(self._h, _ptr(m), _ptr(vals), n, nl, float(scale), sampler_key(key),
                                               stream_id, log2.ctypes.data)
        if rc != 0:
            err = MkckksError(rc, self._L.mkckks_last_error().decode())
            err.log2_sigma = log2
            raise err
        return log2

    def decrypt(self, ct, sk, m, n_ct, nl):
        self._check(self._L.mkckks_decrypt_batch(self._h, _ptr(ct), _ptr(sk), _ptr(m), n_ct, nl))

    def partial_decrypt(self, ct, sk, e, share, n_ct, nl_in, nl, lead):
        """share[t] = INTT(c1 * sk (+ c0 when lead)) + e[t] on the first nl limbs of ct[t]: one party's share of a threshold
        decryption.  e int64 smudging errors (sample_gauss_wide), fresh for every call; exactly one party passes lead."""
        self._check(self._L.mkckks_partial_decrypt_batch(self._h, _ptr(ct), _ptr(sk), _ptr(e), _ptr(share), n_ct, nl_in, nl,
                                                         int(bool(lead))))

    def fuse_shares(self, shares, m, n_parties, n_ct, nl):
        """m = sum of shares[p] (MultipartyDecryptFusion), in the layout of `decrypt`; m may be shares[0]."""
        self._check(self._L.mkckks_fuse_shares_batch(self._h, _ptr(shares), _ptr(m), n_parties, n_ct, nl))

    def switch_share(self, ct, sk, pk, v, e0, e1, nl, lead=False, out=None):
        """One party's share of the collective key switch of ct u64[n_ct][2][nl_in][N] (a joint-key ciphertext batch) to
        the RECIPIENT's public key pk, on the first nl limbs: (c1 * sk (+ c0 when lead) + pk0 * NTT(v) + NTT(e0),
        pk1 * NTT(v) + NTT(e1)), u64[n_ct][2][nl][N], returned (or written to `out`).  v int8 ternary, e0 int64 smudging
        errors, e1 int64 encryption errors, fresh for every call; exactly one party passes lead.  The parties' shares sum
        (eval_sum) to a ciphertext under the recipient's key.  sk may be a key share lambda_j * sigma_j."""
        n_ct, parts, nl_in, n = ct.shape
        if parts != 2 or n != self.N:
            raise ValueError("switch_share: ct must be shaped [n_ct][2][nl_in][N]")
        share = self.empty((n_ct, 2, nl, n), np.uint64) if out is None else out
        self._check(self._L.mkckks_switch_share_batch(self._h, _ptr(ct), _ptr(sk), _ptr(pk), _ptr(v), _ptr(e0), _ptr(e1),
                                                      _ptr(share), n_ct, nl_in, nl, int(bool(lead))))
        return share

    # ---- t-of-n threshold decryption (include/mkckks.h: "t-of-n threshold decryption")
    def share_key(self, sk, shares, nl, n_parties, threshold, key, stream_id=0):
        """shares[p] = sk + sum_{k=1}^{t-1} r_k (p + 1)^k mod q_i on the first nl limbs: the dealer's Shamir sharing of its
        key; r_k = sample_uniform(1, nl, 0, key, stream_id + k - 1), never written.  `key`: a fresh 32-byte key per call."""
        self._check(self._L.mkckks_share_key(self._h, _ptr(sk), _ptr(shares), nl, n_parties, threshold, sampler_key(key),
                                             stream_id))

    def combine_key_shares(self, inp, weights, out, m, nl):
        """out = sum_j weights[j][i] * inp[j][i] mod q_i over m polynomials u64[nl][N]; `weights`: host u64[m][nl] below
        their moduli; out may be inp."""
        w = np.ascontiguousarray(weights, dtype=np.uint64)
        if w.size != m * nl:
            raise ValueError("combine_key_shares: need one weight per input and limb")
        self._check(self._L.mkckks_combine_key_shares(self._h, _ptr(inp), w.ctypes.data, _ptr(out), m, nl))

    def lagrange_at_zero(self, parties):
        """Lagrange coefficients at 0 of the 1-based party indices `parties`: uint64[len(parties)][L] (host only)."""
        p = np.ascontiguousarray(parties, dtype=np.uint32)
        out = np.zeros((p.size, self.L), dtype=np.uint64)
        self._check(self._L.mkckks_lagrange_at_zero(self._h, p.ctypes.data, p.size, out.ctypes.data))
        return out
