"""ctypes binding of libpqhip.so (include/pqhip.h).  Plumbing only -- no compute here."""
import ctypes
import os
import subprocess
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.environ.get("PQHIP_LIB") or os.path.join(_HERE, "libpqhip.so")   # PQHIP_LIB: A/B of two builds on one box (tools/)
_lib = None

OK, EINVAL, ESHAPE, ECODE_RANGE, EINDEX_WIDTH, ENODEV, EHIP, ENOMEM, EUNSUPPORTED = range(9)


class PanicError(AssertionError):
    """A Rust `panic!` / failed `assert!` of the reference surfaced as an exception."""


class PqHipError(RuntimeError):
    def __init__(self, status, what=""):
        self.status = status
        msg = "status %d" % status
        if _lib is not None:
            msg = _lib.pqhip_strerror(status).decode()
            if status == EHIP:
                msg += " [" + _lib.pqhip_last_hip_error().decode() + "]"
        super().__init__("pqhip: %s%s" % (msg, (" (" + what + ")") if what else ""))


def lib_path():
    return _SO


def build(force=False):
    """Compile libpqhip.so for gfx950 (hipcc cross-compiles without a GPU)."""
    srcdir = os.path.join(_HERE, "csrc")
    cmd = ["make", "-C", srcdir, "-s", "-j8"]
    if force:
        cmd.append("-B")
    subprocess.check_call(cmd)
    return _SO


def lib():
    """Load libpqhip.so.  Fails loudly if it is missing: there is no fallback."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_SO):
        raise ImportError("reductive_amd: %s is missing; run reductive_amd.build() "
                          "(needs hipcc). There is no CPU fallback." % _SO)
    # torch bundles its own libamdhip64 (same SONAME).  If torch is going to live in this
    # process it must be loaded first so that both share ONE HIP runtime.
    if "torch" not in sys.modules:
        try:
            import torch  # noqa: F401
        except Exception:  # pragma: no cover - torch is optional for the C ABI itself
            pass
    L = ctypes.CDLL(_SO)
    for name, (restype, argtypes) in SIGNATURES.items():
        f = getattr(L, name)
        f.restype = restype
        f.argtypes = argtypes
    _lib = L
    return L


def _signatures():
    """name -> (restype, argtypes) of every symbol include/pqhip.h declares."""
    i32, i64, vp, cstr = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_char_p
    fp, pi32, pi64, pvp = (ctypes.POINTER(t) for t in (ctypes.c_float, i32, i64, vp))
    sig = {
        "pqhip_version": (i32, []),
        "pqhip_strerror": (cstr, [i32]),
        "pqhip_last_hip_error": (cstr, []),
        "pqhip_device_count": (i32, [pi32]),
        "pqhip_ctx_create": (i32, [pi32, i32, pvp]),
        "pqhip_ctx_destroy": (None, [vp]),
        "pqhip_ctx_n_devices": (i32, [vp]),
        "pqhip_ctx_set_option": (i32, [vp, cstr, i64]),
        "pqhip_codebook_create": (i32, [vp, fp, i64, i64, i64, fp, pvp]),
        "pqhip_codebook_destroy": (None, [vp]),
        "pqhip_codebook_quantized_len": (i64, [vp]),
        "pqhip_codebook_reconstructed_len": (i64, [vp]),
        "pqhip_codebook_n_centroids": (i64, [vp]),
        "pqhip_codebook_has_projection": (i32, [vp]),
        "pqhip_quantize_batch_f32": (i32, [vp, vp, i64, i64, i64, vp, i32, i64, i64]),
        "pqhip_reconstruct_batch_f32": (i32, [vp, vp, i32, i64, i64, i64, vp, i64, i64]),
        "pqhip_quantize_batch_f32_dev": (i32, [vp, i32, vp, i64, i64, vp, i32, i64, vp]),
        "pqhip_reconstruct_batch_f32_dev": (i32, [vp, i32, vp, i32, i64, i64, vp, i64, vp]),
        "pqhip_reconstruct_rows_f32_dev": (i32, [vp, i32, vp, i32, i64, i64, vp, i64, vp, vp, i64, vp]),
        "pqhip_reconstruct_rows_records_f32_dev": (i32, [vp, i32, vp, i32, i64, i64, i64, vp, i64, vp, i64, vp]),
        "pqhip_check_codes_dev": (i32, [vp, i32, vp]),
        "pqhip_adc_tables_f32_dev": (i32, [vp, i32, vp, i64, i64, vp, vp]),
        "pqhip_adc_ip_tables_f32_dev": (i32, [vp, i32, vp, i64, i64, vp, vp]),
        "pqhip_adc_scan_f32_dev": (i32, [vp, i32, vp, i64, vp, i32, i64, i64, vp, i64, vp]),
        "pqhip_pack_codes4_dev": (i32, [vp, i32, vp, i32, i64, i64, vp, i64, vp]),
        "pqhip_unpack_codes4_dev": (i32, [vp, i32, vp, i64, i64, vp, i64, vp, i64, vp]),
        "pqhip_pack_row_mask_dev": (i32, [vp, i32, vp, i64, vp, i64, vp, vp]),
        "pqhip_rerank_f32_dev": (i32, [vp, i32, vp, i64, i64, vp, i32, i64, i64, i64, vp, i32, i64, i32, i32,
                                       vp, i64, vp, i64, vp]),
        "pqhip_flat_search_f32_dev": (i32, [vp, i32, vp, i64, i64, vp, i32, i64, i64, i64, vp, i32, i32,
                                            vp, i64, vp, i64, vp]),
        "pqhip_flat_search_lists_f32_dev": (i32, [vp, i32, vp, i64, i64, vp, i32, i64, i64, i64, vp, i64, vp, i32, i64,
                                                  vp, i32, i32, vp, i64, vp, i64, vp]),
        "pqhip_flat_range_f32_dev": (i32, [vp, i32, vp, i64, i64, vp, i32, i64, i64, i64, vp, i32,
                                           vp, vp, vp, vp, i64, vp]),
        "pqhip_flat_range_lists_f32_dev": (i32, [vp, i32, vp, i64, i64, vp, i32, i64, i64, i64, vp, vp, i64, vp, i32, i64,
                                                 i32, vp, vp, vp, vp, i64, vp]),
        "pqhip_flat_among_f32_dev": (i32, [vp, i32, vp, i64, i64, vp, i32, i64, i64, i64, vp, vp, i64, i32, i32,
                                           vp, i64, vp, i64, vp]),
        "pqhip_flat_range_among_f32_dev": (i32, [vp, i32, vp, i64, i64, vp, i32, i64, i64, i64, vp, vp, i64, i32,
                                                 vp, vp, vp, vp, i64, vp]),
        "pqhip_flat_screen_f32_dev": (i32, [vp, i32, vp, i64, i64, vp, i32, i64, i64, i64, vp, i32, i32,
                                            vp, vp, vp, i64, vp]),
        "pqhip_lists_merge_dev": (i32, [vp, i32, vp, i64, vp, i64, i64, i64, vp, vp, vp, vp, vp]),
        "pqhip_rows_compact_dev": (i32, [vp, i32, vp, i64, i64, vp, vp, i64, vp, i64, vp, vp, vp, vp]),
        "pqhip_topk_merge_f32_dev": (i32, [vp, i32, vp, i64, i64, vp, i64, i64, i64, i64, i32, vp, i32, i32,
                                           vp, i64, vp, i64, vp, i64, vp]),
        "pqhip_lists_layout_dev": (i32, [vp, i32, vp, i32, i64, i64, vp, vp, vp, vp, vp]),
        "pqhip_residuals_f32_dev": (i32, [vp, i32, vp, i64, i64, i64, vp, vp, i64, vp, i64, vp]),
        "pqhip_residual_terms_f32_dev": (i32, [vp, i32, vp, i64, i64, vp, vp, i64, vp, vp]),
        "pqhip_cluster_assignments_f32": (i32, [vp, fp, i64, i64, vp, i64, i64, i64, vp, i32]),
        "pqhip_kmeans_iterations_f32": (i32, [vp, fp, i64, i64, i64, vp, i64, i64, i64, i32, fp]),
        "pqhip_kmeans_iterations_f32_dev": (i32, [vp, i32, fp, i64, i64, i64, vp, i64, i64, i32, fp, vp]),
        "pqhip_opq_train_step_f32_dev": (i32, [vp, i32, fp, i64, i64, i64, fp, vp, i64, i64, fp, vp]),
        "pqhip_at_dot_b_f32_dev": (i32, [vp, i32, vp, i64, i64, vp, i64, i64, i64, fp, vp]),
        "pqhip_rotate_f32_dev": (i32, [vp, i32, vp, i64, i64, i64, fp, vp, i64, vp]),
        "pqhip_matrix_upload_f32": (i32, [vp, i32, vp, i64, i64, i64, i64, pvp]),
        "pqhip_matrix_device_ptr": (vp, [vp]),
        "pqhip_matrix_rows": (i64, [vp]),
        "pqhip_matrix_destroy": (None, [vp]),
        "pqhip_set_encode_variant": (i32, [vp, i32]),
        "pqhip_set_rotation_variant": (i32, [i32]),
        "pqhip_last_encode_kernel": (cstr, [vp]),
        "pqhip_launch_log": (cstr, []),
        "pqhip_launch_log_reset": (None, []),
        "pqhip_vor2_tables_host": (i32, [vp, i64, i64, i64, vp, i64, vp, pi64]),
        "pqhip_selftest_mfma_chain": (i32, [vp, i32, i32, i32, ctypes.c_uint64, pi64]),
    }
    # The 24 ADC search and range entry points follow one grammar (reductive_amd/_marshal.py: search_head builds the
    # same arguments):  cb, slot, tables, nq, codes, [code_bytes], n, codes_row_stride, [mask], [lists], [bias], [last],
    # then the outputs.  plain: no mask; masked and range: the mask; packed4: the mask and no code_bytes.
    lists = [vp, i64, vp, i32, i64]                 # list_off, n_lists, probes, n_probe, probes_row_stride
    bias = [vp, i64]                                # probe_bias, probe_bias_row_stride
    topk = [i32, vp, i64, vp, i64, vp]              # k, val, val_row_stride, idx, idx_row_stride, stream
    csr = [vp, vp, vp, vp, i64, vp]                 # threshold, lims, val, idx, capacity, stream
    for ip in ("", "ip_"):
        for where, mid in (("", []), ("_lists", lists), ("_lists_residual", lists + bias)):
            if ip or where == "_lists_residual":    # last: the scales of a similarity search, else the row terms
                mid = mid + [vp]
            search, rng = "pqhip_adc_%ssearch%s" % (ip, where), "pqhip_adc_%srange%s_f32_dev" % (ip, where)
            sig[search + "_f32_dev"] = (i32, [vp, i32, vp, i64, vp, i32, i64, i64] + mid + topk)
            sig[search + "_masked_f32_dev"] = (i32, [vp, i32, vp, i64, vp, i32, i64, i64, vp] + mid + topk)
            sig[search + "_packed4_f32_dev"] = (i32, [vp, i32, vp, i64, vp, i64, i64, vp] + mid + topk)
            sig[rng] = (i32, [vp, i32, vp, i64, vp, i32, i64, i64, vp] + mid + csr)
    # The two searches among given rows: lims, ids, n_ids; row_list, n_lists; list_bias, its row stride; row terms / scales
    for name in ("pqhip_adc_among_f32_dev", "pqhip_adc_ip_among_f32_dev"):
        sig[name] = (i32, [vp, i32, vp, i64, vp, i32, i64, i64, vp, vp, i64, vp, i64, vp, i64, vp] + topk)
    return sig


SIGNATURES = _signatures()
EXPORTS = list(SIGNATURES)      # every symbol include/pqhip.h declares (checked by the CPU test-suite)
