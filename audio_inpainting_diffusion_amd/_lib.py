"""ctypes binding of libaid_hip.so: the C ABI of the headers under include/, one entry of ``ABIS`` each (the table below the struct mirrors;
``lib()`` binds from it and tests/test_abi_host.py holds it to the headers, field by field).

There is deliberately NO fallback: if the shared library is missing or a launcher returns an error code,
``AidError`` is raised.  Tensors are passed as raw device pointers + element strides; the stream is torch's
current HIP stream, so kernels order naturally with torch allocations/copies and can be graph-captured.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, NamedTuple, Optional, Sequence, Tuple

import torch

from . import winograd

_HERE = os.path.dirname(os.path.abspath(__file__))
# (AID_LIB_PATH selects another build of the library for kernel A/B experiments -- honoured only together with AID_EXPERIMENT=1, and announced on
#  stderr, so that a stray variable can never silently change what a run measures)
LIB_PATH = os.path.join(_HERE, "libaid_hip.so")
if os.environ.get("AID_EXPERIMENT") == "1" and os.environ.get("AID_LIB_PATH"):
    LIB_PATH = os.environ["AID_LIB_PATH"]
    import sys as _sys
    print(f"[aid] AID_EXPERIMENT=1: loading {LIB_PATH} instead of the in-tree libaid_hip.so", file=_sys.stderr)
# (the AID_* constants of this module that repeat a #define are listed per header in ABIS[...].macros and compared with it by tests/test_abi_host.py)
AID_CQT_MAX_OCT = 12
AID_STATS_SPLIT = 32
AID_CONV2D_SPLIT_FLAG_BYTES = 4096     # leading flag region of the split-K scratch
AID_ATTN_MAX_T = 128          # aid_time_attention: one workgroup holds a whole [T, T] score tile
AID_ATTN_LONG_MAX_T = 1024    # aid_time_attention_long: a wave holds one 32-key tile of each of up to eight 128-key chunks


class AidError(RuntimeError):
    pass


class View(C.Structure):
    _fields_ = [("p", C.c_void_p), ("sB", C.c_int64), ("sC", C.c_int64), ("sF", C.c_int64)]


class GroupStatsParams(C.Structure):
    _fields_ = [("x", View), ("B", C.c_int), ("C", C.c_int), ("F", C.c_int), ("T", C.c_int), ("groups", C.c_int),
                ("gamma", C.c_void_p), ("mod", C.c_void_p), ("mod_ld", C.c_int64), ("eps", C.c_float),
                ("scale", C.c_void_p), ("stats", C.c_void_p), ("ws", C.c_void_p), ("ws_n", C.c_int)]


class Conv2dParams(C.Structure):
    _fields_ = [("x", View), ("y", View), ("res", View), ("aux", View),
                ("wp", C.c_void_p),
                ("in_scale", C.c_void_p), ("in_scale_ld", C.c_int64),
                ("out_scale", C.c_void_p), ("out_scale_ld", C.c_int64),
                ("aux_scale", C.c_void_p), ("aux_scale_ld", C.c_int64),
                ("B", C.c_int), ("Cin", C.c_int), ("Cout", C.c_int), ("F", C.c_int), ("T", C.c_int),
                ("Cin_pad", C.c_int), ("Cout_pad", C.c_int),
                ("KH", C.c_int), ("KW", C.c_int), ("dilF", C.c_int),
                ("act", C.c_int), ("epi", C.c_int),
                ("alpha", C.c_float), ("res_scale", C.c_float), ("wp_wino", C.c_void_p), ("wino_taps", C.c_int),
                ("x_wino", C.c_int), ("ws", C.c_void_p), ("ws_bytes", C.c_int64),
                ("dot_ws", C.c_void_p), ("dot_n", C.c_int), ("stat_ws", C.c_void_p), ("stat_n", C.c_int),
                ("x2", View), ("Cin1", C.c_int),
                ("fin_mode", C.c_int), ("fin_count", C.c_void_p), ("fin_gamma", C.c_void_p), ("fin_mod", C.c_void_p), ("fin_mod_ld", C.c_int64),
                ("fin_eps", C.c_float), ("fin_scale", C.c_void_p), ("fin_stats", C.c_void_p)]


class Wino2dGemmParams(C.Structure):
    _fields_ = [("U", C.c_void_p), ("V", C.c_void_p), ("M", C.c_void_p), ("nxi", C.c_int), ("Cin", C.c_int), ("Cout", C.c_int),
                ("Cin_pad", C.c_int), ("Cout_pad", C.c_int), ("N", C.c_int64), ("variant", C.c_int)]


class ResampleParams(C.Structure):
    _fields_ = [("x", View), ("y", View), ("B", C.c_int), ("C", C.c_int), ("F", C.c_int), ("T", C.c_int),
                ("up", C.c_int), ("adjoint", C.c_int), ("accumulate", C.c_int)]


class AttentionParams(C.Structure):
    _fields_ = [("qk", C.c_void_p), ("v", C.c_void_p), ("out", C.c_void_p), ("probs", C.c_void_p),
                ("B", C.c_int), ("H", C.c_int), ("F", C.c_int), ("T", C.c_int), ("scale", C.c_float), ("bias", C.c_void_p)]


class EmbedParams(C.Structure):
    _fields_ = [("sigma", C.c_void_p), ("rff_freq", C.c_void_p), ("w0", C.c_void_p), ("b0", C.c_void_p),
                ("w1", C.c_void_p), ("b1", C.c_void_p), ("w2", C.c_void_p), ("b2", C.c_void_p), ("emb", C.c_void_p),
                ("B", C.c_int), ("rff", C.c_int), ("h0", C.c_int), ("h1", C.c_int), ("E", C.c_int)]


class ModulationParams(C.Structure):
    _fields_ = [("emb", C.c_void_p), ("W", C.c_void_p), ("bias", C.c_void_p), ("mod", C.c_void_p),
                ("B", C.c_int), ("E", C.c_int), ("N", C.c_int)]


class CqtTables(C.Structure):
    _fields_ = [("n_oct", C.c_int), ("bins", C.c_int), ("rc", C.c_void_p), ("Lg", C.c_void_p), ("goff", C.c_void_p),
                ("g", C.c_void_p), ("T_oct", C.c_void_p), ("twiddle", C.c_void_p), ("Tmax", C.c_int)]


class CqtParams(C.Structure):
    _fields_ = [("tab", CqtTables), ("T_host", C.c_int * AID_CQT_MAX_OCT), ("oct", View * AID_CQT_MAX_OCT),
                ("spec", C.c_void_p), ("band_ws", C.c_void_p), ("in_scale", C.c_void_p), ("B", C.c_int), ("Lh", C.c_int),
                ("unnormalized", C.c_int)]


class CqtGatherParams(C.Structure):
    _fields_ = [("band_ws", C.c_void_p), ("kfirst", C.c_void_p), ("kcount", C.c_void_p),
                ("rc", C.c_void_p), ("Lg", C.c_void_p), ("goff", C.c_void_p), ("woff", C.c_void_p), ("Tk", C.c_void_p),
                ("gdM", C.c_void_p), ("X", C.c_void_p), ("cskip", C.c_void_p), ("cout", C.c_void_p), ("hpf", C.c_void_p),
                ("Y", C.c_void_p), ("B", C.c_int), ("Lh", C.c_int), ("ws_per_b", C.c_int64), ("band_scale", C.c_void_p)]


class AxpbyParams(C.Structure):
    _fields_ = [("x", C.c_void_p), ("y", C.c_void_p), ("out", C.c_void_p), ("a", C.c_void_p), ("b", C.c_void_p),
                ("B", C.c_int), ("L", C.c_int64), ("a_host", C.c_float), ("b_host", C.c_float)]

    def __init__(self, x, y, out, a, b, B, L, a_host=1.0, b_host=1.0):
        super().__init__(x, y, out, a, b, B, L, a_host, b_host)


class ScoreStepParams(C.Structure):
    _fields_ = [("x", C.c_void_p), ("xhat", C.c_void_p), ("yobs", C.c_void_p), ("smask", C.c_void_p),
                ("smask_sB", C.c_int64), ("x0", C.c_void_p), ("d0", C.c_void_p), ("t", C.c_void_p), ("h", C.c_void_p),
                ("xnext", C.c_void_p), ("dout", C.c_void_p), ("xh_out", C.c_void_p),
                ("B", C.c_int), ("L", C.c_int64), ("mode", C.c_int), ("t_host", C.c_float), ("h_host", C.c_float)]


class Add2Params(C.Structure):
    _fields_ = [("u", View), ("v", View), ("y", View), ("B", C.c_int), ("C", C.c_int), ("F", C.c_int), ("T", C.c_int),
                ("a", C.c_float), ("b", C.c_float)]


class ScaleActParams(C.Structure):
    _fields_ = [("x", View), ("y", View), ("scale", C.c_void_p), ("scale_ld", C.c_int64),
                ("B", C.c_int), ("C", C.c_int), ("F", C.c_int), ("T", C.c_int), ("act", C.c_int), ("wino", C.c_int), ("dilF", C.c_int), ("mul", C.c_float)]


class FftPassParams(C.Structure):
    _fields_ = [("inp", C.c_void_p), ("out", C.c_void_p), ("twiddle", C.c_void_p), ("B", C.c_int), ("N", C.c_int), ("R", C.c_int),
                ("Ns", C.c_int), ("in_mode", C.c_int), ("out_mode", C.c_int), ("sign", C.c_float), ("out_scale", C.c_float)]


class GroupDotParams(C.Structure):
    _fields_ = [("u", View), ("v", View), ("B", C.c_int), ("C", C.c_int), ("F", C.c_int), ("T", C.c_int), ("groups", C.c_int),
                ("ws", C.c_void_p)]


class NormBwdParams(C.Structure):
    _fields_ = [("gd", View), ("x", View), ("gy", View), ("out", View),
                ("B", C.c_int), ("C", C.c_int), ("F", C.c_int), ("T", C.c_int), ("groups", C.c_int),
                ("stats", C.c_void_p), ("ws", C.c_void_p), ("eps", C.c_float), ("a", C.c_float), ("accumulate", C.c_int),
                ("ws_n", C.c_int), ("wout", View), ("wscale", C.c_void_p), ("wscale_ld", C.c_int64), ("wform", C.c_int), ("coef_ready", C.c_int), ("wdil", C.c_int)]


class AttentionBwdParams(C.Structure):
    _fields_ = [("qk", C.c_void_p), ("v", C.c_void_p), ("probs", C.c_void_p), ("gout", C.c_void_p),
                ("gqk", C.c_void_p), ("gv", C.c_void_p), ("B", C.c_int), ("H", C.c_int), ("F", C.c_int), ("T", C.c_int),
                ("scale", C.c_float), ("accumulate_gv", C.c_int), ("ws", C.c_void_p)]


class GuidanceSeedParams(C.Structure):
    _fields_ = [("xhat", C.c_void_p), ("y", C.c_void_p), ("mask", C.c_void_p), ("mask_sB", C.c_int64),
                ("g", C.c_void_p), ("norm", C.c_void_p), ("B", C.c_int), ("L", C.c_int64), ("norm_type", C.c_int), ("beta", C.c_float)]

    def __init__(self, xhat, y, mask, mask_sB, g, norm, B, L, norm_type=2, beta=1.0):
        super().__init__(xhat, y, mask, mask_sB, g, norm, B, L, norm_type, beta)


class GuidanceStepParams(C.Structure):
    _fields_ = [("xhat", C.c_void_p), ("g", C.c_void_p), ("out", C.c_void_p), ("step_out", C.c_void_p), ("s_out", C.c_void_p),
                ("B", C.c_int), ("L", C.c_int64), ("coef", C.c_float), ("inv_sqrt_len", C.c_float), ("eps", C.c_float)]


class SetRowsParams(C.Structure):
    _fields_ = [("out", C.c_void_p), ("ld", C.c_int64), ("B", C.c_int), ("n", C.c_int), ("v", C.c_float * 8)]


class RowNormParams(C.Structure):
    _fields_ = [("x", C.c_void_p), ("out", C.c_void_p), ("B", C.c_int), ("L", C.c_int64)]


class ResamplePolyParams(C.Structure):
    _fields_ = [("x", C.c_void_p), ("y", C.c_void_p), ("kernel", C.c_void_p), ("x_ld", C.c_int64), ("y_ld", C.c_int64),
                ("L", C.c_int64), ("Lout", C.c_int64), ("B", C.c_int), ("orig_freq", C.c_int), ("new_freq", C.c_int),
                ("width", C.c_int), ("K", C.c_int)]


class StftParams(C.Structure):
    _fields_ = [("x", C.c_void_p), ("frames", C.c_void_p), ("out", C.c_void_p),
                ("window", C.c_void_p), ("twiddle", C.c_void_p), ("inv_env", C.c_void_p),
                ("mask", C.c_void_p), ("mask_sB", C.c_int64), ("mask_ld", C.c_int64),
                ("add1", C.c_void_p), ("add2", C.c_void_p), ("c0", C.c_float),
                ("B", C.c_int), ("L", C.c_int64), ("Lp", C.c_int64),
                ("n_fft", C.c_int), ("hop", C.c_int), ("n_frames", C.c_int), ("adjoint", C.c_int)]


class WgradParams(C.Structure):
    _fields_ = [("gy", View), ("x", View), ("P", C.c_void_p),
                ("B", C.c_int), ("Cin", C.c_int), ("Cout", C.c_int), ("F", C.c_int), ("T", C.c_int), ("KH", C.c_int), ("KW", C.c_int),
                ("dilF", C.c_int), ("S", C.c_int), ("alpha", C.c_float), ("wino", C.c_int)]


class WinoGyParams(C.Structure):
    _fields_ = [("gy", View), ("out", View), ("B", C.c_int), ("C", C.c_int), ("F", C.c_int), ("T", C.c_int)]


class PackConvWeightParams(C.Structure):
    _fields_ = [("w", C.c_void_p), ("wp", C.c_void_p), ("wpT", C.c_void_p), ("wpw", C.c_void_p), ("wpwT", C.c_void_p),
                ("Cout", C.c_int), ("Cin", C.c_int), ("KH", C.c_int), ("KW", C.c_int),
                ("Cin_pad", C.c_int), ("Cout_pad", C.c_int), ("Cin_padT", C.c_int), ("Cout_padT", C.c_int),
                ("wpw8", C.c_void_p), ("wpw8T", C.c_void_p), ("wpw2", C.c_void_p), ("wpw2T", C.c_void_p), ("wpw3", C.c_void_p), ("wpw3T", C.c_void_p)]


class WgradReduceParams(C.Structure):
    _fields_ = [("P", C.c_void_p), ("W", C.c_void_p), ("gate", C.c_void_p), ("gate_ld", C.c_int64),
                ("in_scale", C.c_void_p), ("in_scale_ld", C.c_int64), ("dW", C.c_void_p), ("dgate", C.c_void_p), ("dgate_ld", C.c_int64),
                ("B", C.c_int), ("S", C.c_int), ("Cout", C.c_int), ("Cin", C.c_int), ("K", C.c_int), ("accumulate", C.c_int),
                ("wino", C.c_int), ("Uw", C.c_void_p), ("Cin_pad", C.c_int), ("Cout_pad", C.c_int)]


class ChannelDotParams(C.Structure):
    _fields_ = [("u", View), ("v", View), ("out", C.c_void_p), ("out_ld", C.c_int64),
                ("B", C.c_int), ("C", C.c_int), ("F", C.c_int), ("T", C.c_int)]


class RelposBwdParams(C.Structure):
    _fields_ = [("dS", C.c_void_p), ("bucket", C.c_void_p), ("dW", C.c_void_p),
                ("B", C.c_int), ("H", C.c_int), ("T", C.c_int), ("num_buckets", C.c_int), ("accumulate", C.c_int)]


class ScaleBwdParams(C.Structure):
    _fields_ = [("S", C.c_void_p), ("S_ld", C.c_int64), ("scale", C.c_void_p), ("scale_ld", C.c_int64), ("gamma", C.c_void_p),
                ("mod", C.c_void_p), ("mod_ld", C.c_int64), ("stats", C.c_void_p), ("dgamma", C.c_void_p), ("dmod", C.c_void_p),
                ("dmod_ld", C.c_int64), ("B", C.c_int), ("C", C.c_int), ("groups", C.c_int), ("accumulate", C.c_int)]


class ModulationBwdParams(C.Structure):
    _fields_ = [("dmod", C.c_void_p), ("emb", C.c_void_p), ("W", C.c_void_p), ("dW", C.c_void_p), ("dbias", C.c_void_p),
                ("demb", C.c_void_p), ("B", C.c_int), ("E", C.c_int), ("N", C.c_int), ("accumulate", C.c_int),
                ("part", C.c_void_p), ("part_floats", C.c_int64)]


class EmbedBwdParams(C.Structure):
    _fields_ = [("fwd", EmbedParams), ("demb", C.c_void_p), ("dw0", C.c_void_p), ("db0", C.c_void_p), ("dw1", C.c_void_p),
                ("db1", C.c_void_p), ("dw2", C.c_void_p), ("db2", C.c_void_p), ("accumulate", C.c_int)]


class AdamParams(C.Structure):
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("gscale", C.c_void_p),
                ("n", C.c_int64), ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float),
                ("bias1", C.c_float), ("bias2_sqrt", C.c_float)]


class EmaParams(C.Structure):
    _fields_ = [("dst", C.c_void_p), ("src", C.c_void_p), ("n", C.c_int64), ("rate", C.c_float)]


class SumsqParams(C.Structure):
    _fields_ = [("x", C.c_void_p), ("ws", C.c_void_p), ("out", C.c_void_p), ("n", C.c_int64), ("max_norm", C.c_float)]


AID_SUMSQ_BLOCKS = 512


# ---- include/aid_degrade.h (restoration degradations) ----
class FirParams(C.Structure):
    _fields_ = [("x", C.c_void_p), ("out", C.c_void_p), ("h", C.c_void_p), ("add1", C.c_void_p), ("add2", C.c_void_p), ("c0", C.c_float),
                ("B", C.c_int), ("K", C.c_int), ("stride", C.c_int), ("pad_left", C.c_int), ("adjoint", C.c_int),
                ("L", C.c_int64), ("L_out", C.c_int64), ("x_ld", C.c_int64), ("out_ld", C.c_int64)]


class IirParams(C.Structure):
    _fields_ = [("x", C.c_void_p), ("out", C.c_void_p), ("pre", C.c_void_p), ("coef", C.c_void_p), ("H", C.c_void_p),
                ("z", C.c_void_p), ("state", C.c_void_p), ("add1", C.c_void_p), ("add2", C.c_void_p), ("c0", C.c_float),
                ("B", C.c_int), ("N", C.c_int), ("C", C.c_int), ("clamp", C.c_int), ("adjoint", C.c_int),
                ("L", C.c_int64), ("x_ld", C.c_int64), ("out_ld", C.c_int64)]


class ClipParams(C.Structure):
    _fields_ = [("x", C.c_void_p), ("xref", C.c_void_p), ("out", C.c_void_p), ("add1", C.c_void_p), ("add2", C.c_void_p),
                ("c0", C.c_float), ("clip", C.c_float), ("B", C.c_int), ("adjoint", C.c_int),
                ("L", C.c_int64), ("x_ld", C.c_int64), ("out_ld", C.c_int64)]




# ---- include/aid_phase.h (phase retrieval: STFT magnitude and the induced-matrix-norm seed) ----
class StftMagParams(C.Structure):
    _fields_ = [("x", C.c_void_p), ("g", C.c_void_p), ("out", C.c_void_p), ("frames", C.c_void_p), ("window", C.c_void_p), ("twiddle", C.c_void_p),
                ("B", C.c_int), ("n_fft", C.c_int), ("hop", C.c_int), ("n_frames", C.c_int), ("adjoint", C.c_int),
                ("L", C.c_int64), ("x_ld", C.c_int64), ("out_ld", C.c_int64)]


class MatrixNormParams(C.Structure):
    _fields_ = [("den", C.c_void_p), ("y", C.c_void_p), ("g", C.c_void_p), ("norm", C.c_void_p), ("r", C.c_void_p), ("diag", C.c_void_p),
                ("B", C.c_int), ("F", C.c_int), ("T", C.c_int), ("ord", C.c_int), ("max_iter", C.c_int), ("tol", C.c_double)]



# ---- include/aid_autoregressive.h (the window carry of autoregressive generation) ----
class ArCarryParams(C.Structure):
    _fields_ = [("x", C.c_void_p), ("y", C.c_void_p), ("out", C.c_void_p), ("B", C.c_int), ("first", C.c_int),
                ("L", C.c_int64), ("end", C.c_int64), ("off", C.c_int64), ("out_ld", C.c_int64)]




# ---- include/aid_restore.h (window gather / scatter of whole-recording restoration) ----
class WindowGatherParams(C.Structure):
    _fields_ = [("rec", C.c_void_p), ("out", C.c_void_p), ("mask", C.c_void_p), ("y", C.c_void_p), ("m", C.c_void_p), ("jobs", C.c_void_p),
                ("J", C.c_int), ("R", C.c_int), ("L", C.c_int64), ("N", C.c_int64), ("rec_ld", C.c_int64), ("out_ld", C.c_int64), ("mask_ld", C.c_int64)]


class WindowScatterParams(C.Structure):
    _fields_ = [("x", C.c_void_p), ("out", C.c_void_p), ("jobs", C.c_void_p), ("J", C.c_int), ("R", C.c_int),
                ("L", C.c_int64), ("N", C.c_int64), ("out_ld", C.c_int64)]


AID_RESTORE_JOB_FIELDS = 6             # r, s, head, tail, lo, hi (int64 each)

# ---- include/aid_declip.h (declipping whole recordings: the clipped / known / absent operator and its gather) ----
class ClipKnownParams(C.Structure):
    _fields_ = [("x", C.c_void_p), ("xref", C.c_void_p), ("y", C.c_void_p), ("state", C.c_void_p), ("clip", C.c_void_p), ("out", C.c_void_p),
                ("B", C.c_int), ("mode", C.c_int), ("L", C.c_int64), ("x_ld", C.c_int64), ("xref_ld", C.c_int64), ("y_ld", C.c_int64),
                ("state_ld", C.c_int64), ("out_ld", C.c_int64)]


class DeclipGatherParams(C.Structure):
    _fields_ = [("rec", C.c_void_p), ("out", C.c_void_p), ("clip", C.c_void_p), ("y", C.c_void_p), ("k", C.c_void_p), ("c", C.c_void_p), ("jobs", C.c_void_p),
                ("J", C.c_int), ("R", C.c_int), ("L", C.c_int64), ("N", C.c_int64), ("rec_ld", C.c_int64), ("out_ld", C.c_int64)]



# ---- include/aid_resample_op.h (the resampling degradation of bandwidth extension: the adjoint of aid_resample_poly) ----
class ResamplePolyAdjParams(C.Structure):
    _fields_ = [("g", C.c_void_p), ("gx", C.c_void_p), ("kT", C.c_void_p), ("j_lo", C.c_void_p), ("j_hi", C.c_void_p),
                ("g_ld", C.c_int64), ("gx_ld", C.c_int64), ("L", C.c_int64), ("Lout", C.c_int64),
                ("B", C.c_int), ("orig_freq", C.c_int), ("new_freq", C.c_int), ("width", C.c_int), ("K", C.c_int)]



# ---- include/aid_bwe_long.h (bandwidth extension of whole recordings: the filtered / known / unobserved / absent FIR operator and its gather) ----
class FirObservedParams(C.Structure):
    _fields_ = [("x", C.c_void_p), ("y", C.c_void_p), ("state", C.c_void_p), ("h", C.c_void_p), ("out", C.c_void_p),
                ("B", C.c_int), ("K", C.c_int), ("mode", C.c_int), ("L", C.c_int64), ("x_ld", C.c_int64), ("y_ld", C.c_int64),
                ("state_ld", C.c_int64), ("out_ld", C.c_int64)]


class BweGatherParams(C.Structure):
    _fields_ = [("rec", C.c_void_p), ("out", C.c_void_p), ("y", C.c_void_p), ("state", C.c_void_p), ("jobs", C.c_void_p),
                ("J", C.c_int), ("R", C.c_int), ("K", C.c_int), ("L", C.c_int64), ("N", C.c_int64), ("rec_ld", C.c_int64), ("out_ld", C.c_int64)]



# ---- include/aid_lowrate_long.h (bandwidth extension of whole low-sample-rate recordings: the known / observed / unobserved / absent resampling operator and its gather) ----
class RateObservedParams(C.Structure):
    _fields_ = [("x", C.c_void_p), ("state", C.c_void_p), ("k", C.c_void_p), ("kT", C.c_void_p), ("j_lo", C.c_void_p), ("j_hi", C.c_void_p), ("out", C.c_void_p),
                ("L", C.c_int64), ("Mw", C.c_int64), ("x_ld", C.c_int64), ("state_ld", C.c_int64), ("out_ld", C.c_int64),
                ("B", C.c_int), ("mode", C.c_int), ("orig_freq", C.c_int), ("new_freq", C.c_int), ("width", C.c_int), ("K", C.c_int)]


class LowrateGatherParams(C.Structure):
    _fields_ = [("rec", C.c_void_p), ("out", C.c_void_p), ("y", C.c_void_p), ("state", C.c_void_p), ("jobs", C.c_void_p),
                ("L", C.c_int64), ("Mw", C.c_int64), ("N", C.c_int64), ("M", C.c_int64), ("rec_ld", C.c_int64), ("out_ld", C.c_int64),
                ("J", C.c_int), ("R", C.c_int), ("orig_freq", C.c_int), ("new_freq", C.c_int), ("width", C.c_int), ("K", C.c_int)]



# ---- include/aid_phase_long.h (phase retrieval of whole recordings: the known / observed / unobserved / absent STFT-magnitude operator and its gather) ----
class StftMagObservedParams(C.Structure):
    _fields_ = [("x", C.c_void_p), ("g", C.c_void_p), ("state", C.c_void_p), ("window", C.c_void_p), ("twiddle", C.c_void_p), ("frames", C.c_void_p), ("out", C.c_void_p),
                ("L", C.c_int64), ("x_ld", C.c_int64), ("g_ld", C.c_int64), ("state_ld", C.c_int64), ("out_ld", C.c_int64),
                ("B", C.c_int), ("n_fft", C.c_int), ("hop", C.c_int), ("n_frames", C.c_int), ("mode", C.c_int)]


class PrGatherParams(C.Structure):
    _fields_ = [("rec", C.c_void_p), ("out", C.c_void_p), ("y", C.c_void_p), ("state", C.c_void_p), ("jobs", C.c_void_p),
                ("L", C.c_int64), ("N", C.c_int64), ("T_rec", C.c_int64), ("rec_ld", C.c_int64), ("rec_bin_ld", C.c_int64), ("out_ld", C.c_int64),
                ("J", C.c_int), ("R", C.c_int), ("n_fft", C.c_int), ("hop", C.c_int), ("n_frames", C.c_int)]



# ---- include/aid_spec_long.h (spectrogram inpainting of whole recordings: the known / observed / unobserved / absent STFT-masking operator and its gather) ----
class StftMaskObservedParams(C.Structure):
    _fields_ = [("x", C.c_void_p), ("y", C.c_void_p), ("state", C.c_void_p), ("items", C.c_void_p),
                ("window", C.c_void_p), ("twiddle", C.c_void_p), ("inv_env", C.c_void_p), ("mask", C.c_void_p),
                ("frames", C.c_void_p), ("out", C.c_void_p),
                ("L", C.c_int64), ("Np", C.c_int64), ("x_ld", C.c_int64), ("y_ld", C.c_int64), ("state_ld", C.c_int64), ("out_ld", C.c_int64),
                ("mask_sB", C.c_int64), ("mask_ld", C.c_int64),
                ("B", C.c_int), ("Rm", C.c_int), ("n_fft", C.c_int), ("hop", C.c_int), ("n_frames", C.c_int), ("mode", C.c_int)]


class SpecGatherParams(C.Structure):
    _fields_ = [("rec", C.c_void_p), ("out", C.c_void_p), ("y", C.c_void_p), ("state", C.c_void_p), ("items", C.c_void_p), ("jobs", C.c_void_p),
                ("L", C.c_int64), ("N", C.c_int64), ("Np", C.c_int64), ("rec_ld", C.c_int64), ("out_ld", C.c_int64),
                ("J", C.c_int), ("R", C.c_int), ("n_fft", C.c_int), ("hop", C.c_int), ("n_frames", C.c_int)]


AID_SPEC_ITEM_FIELDS = 3

AID_LOWPASS_FIT_MAX_ITEMS = 256        # aid_lowpass_fit_groups: the group ids of a launch travel in the kernel arguments


class Abi(NamedTuple):
    """One header under include/ as the binding sees it.  Adding a header, a struct or an export is one edit here: ``lib()`` binds from this table and
    tests/test_abi_host.py compares every entry with the header (struct set, field order, sizes and offsets, prototypes, version, macros)."""
    header: str                                   # file under include/
    version_fn: str                               # int f(void); its upper-cased name is the header's version #define
    version: int                                  # the version this binding was written against
    structs: Dict[str, type]                      # C typedef name -> ctypes mirror
    launches: Dict[str, type]                     # entry point int f(const params*, void* stream) -> the mirror of its params
    queries: Dict[str, Tuple] = {}                # host functions with signatures of their own: name -> (restype, argtypes)
    macros: Tuple[str, ...] = ()                  # #defines whose value a module constant of the same name repeats

    @property
    def exports(self):
        return [self.version_fn, *self.queries, *self.launches]


def _ints(n):
    return [C.c_int] * n


ABIS = (
    Abi("aid_kernels.h", "aid_abi_version", 14,
        structs={"aid_view": View, "aid_group_stats_params": GroupStatsParams, "aid_conv2d_params": Conv2dParams, "aid_wino2d_gemm_params": Wino2dGemmParams,
                 "aid_resample_params": ResampleParams, "aid_attention_params": AttentionParams, "aid_embed_params": EmbedParams,
                 "aid_modulation_params": ModulationParams, "aid_cqt_tables": CqtTables, "aid_cqt_params": CqtParams, "aid_cqt_gather_params": CqtGatherParams,
                 "aid_fft_pass_params": FftPassParams, "aid_axpby_params": AxpbyParams, "aid_score_step_params": ScoreStepParams,
                 "aid_group_dot_params": GroupDotParams, "aid_norm_bwd_params": NormBwdParams, "aid_attention_bwd_params": AttentionBwdParams,
                 "aid_guidance_seed_params": GuidanceSeedParams, "aid_guidance_step_params": GuidanceStepParams, "aid_set_rows_params": SetRowsParams,
                 "aid_row_norm_params": RowNormParams, "aid_resample_poly_params": ResamplePolyParams, "aid_stft_params": StftParams,
                 "aid_scale_act_params": ScaleActParams, "aid_add2_params": Add2Params, "aid_conv2d_wgrad_params": WgradParams,
                 "aid_wino_gy_params": WinoGyParams, "aid_pack_conv_weight_params": PackConvWeightParams, "aid_wgrad_reduce_params": WgradReduceParams,
                 "aid_channel_dot_params": ChannelDotParams, "aid_relpos_bwd_params": RelposBwdParams, "aid_scale_bwd_params": ScaleBwdParams,
                 "aid_modulation_bwd_params": ModulationBwdParams, "aid_embed_bwd_params": EmbedBwdParams, "aid_adam_params": AdamParams,
                 "aid_ema_params": EmaParams, "aid_sumsq_params": SumsqParams},
        launches={"aid_group_stats": GroupStatsParams, "aid_conv2d": Conv2dParams, "aid_wino2d_gemm": Wino2dGemmParams,
                  "aid_conv2d_wino2d_gemm": Conv2dParams, "aid_conv2d_wino2d_output": Conv2dParams, "aid_resample": ResampleParams,
                  "aid_time_attention": AttentionParams, "aid_embed": EmbedParams, "aid_modulation": ModulationParams,
                  "aid_cqt_analysis": CqtParams, "aid_cqt_synthesis": CqtParams, "aid_cqt_gather": CqtGatherParams, "aid_fft_pass": FftPassParams,
                  "aid_axpby": AxpbyParams, "aid_score_step": ScoreStepParams, "aid_group_dot": GroupDotParams, "aid_norm_bwd": NormBwdParams,
                  "aid_time_attention_bwd": AttentionBwdParams, "aid_guidance_seed": GuidanceSeedParams, "aid_guidance_step": GuidanceStepParams,
                  "aid_set_rows": SetRowsParams, "aid_row_norm": RowNormParams, "aid_resample_poly": ResamplePolyParams,
                  "aid_stft_frames": StftParams, "aid_stft_ola": StftParams, "aid_scale_act": ScaleActParams, "aid_add2": Add2Params,
                  "aid_conv2d_wgrad": WgradParams, "aid_wino_gy": WinoGyParams, "aid_pack_conv_weight": PackConvWeightParams,
                  "aid_wgrad_reduce": WgradReduceParams, "aid_channel_dot": ChannelDotParams, "aid_relpos_bwd": RelposBwdParams,
                  "aid_scale_bwd": ScaleBwdParams, "aid_modulation_bwd": ModulationBwdParams, "aid_embed_bwd": EmbedBwdParams,
                  "aid_adam": AdamParams, "aid_ema": EmaParams, "aid_sumsq": SumsqParams,
                  "aid_time_attention_long": AttentionParams, "aid_time_attention_long_bwd": AttentionBwdParams},
        queries={"aid_last_error": (C.c_char_p, []), "aid_last_kernel": (C.c_char_p, []),
                 "aid_conv2d_pack_dims": (None, [C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
                 "aid_conv2d_wino_input_supported": (C.c_int, _ints(3)), "aid_conv2d_wino_input_ok": (C.c_int, _ints(6)),
                 "aid_conv2d_wino_form": (C.c_int, _ints(6)), "aid_conv2d_wino8_supported": (C.c_int, _ints(5)),
                 "aid_conv2d_wino_split_ws_bytes": (C.c_int64, _ints(6)), "aid_conv2d_fin_supported": (C.c_int, _ints(7)),
                 "aid_conv2d_dot_partials": (C.c_int, _ints(7)), "aid_conv2d_dot_partials_1x1": (C.c_int, _ints(5)),
                 "aid_conv2d_stat_partials": (C.c_int, _ints(7)), "aid_conv2d_x2_supported": (C.c_int, _ints(5)),
                 "aid_conv2d_wgrad_tiles": (C.c_int, _ints(5)), "aid_conv2d_wino2d_supported": (C.c_int, _ints(5)),
                 "aid_conv2d_wino2d_positions": (C.c_int64, _ints(4)), "aid_conv2d_wino2d_wanted": (C.c_int, _ints(6)),
                 "aid_conv2d_wino2d_tform": (C.c_int, _ints(6)), "aid_wino2d_set_split": (C.c_int, _ints(1))},
        macros=("AID_CQT_MAX_OCT", "AID_STATS_SPLIT", "AID_CONV2D_SPLIT_FLAG_BYTES", "AID_SUMSQ_BLOCKS", "AID_ATTN_LONG_MAX_T")),
    Abi("aid_degrade.h", "aid_degrade_abi_version", 1,
        structs={"aid_fir_params": FirParams, "aid_iir_params": IirParams, "aid_clip_params": ClipParams},
        launches={"aid_fir": FirParams, "aid_iir": IirParams, "aid_clip": ClipParams}),
    Abi("aid_phase.h", "aid_phase_abi_version", 1,
        structs={"aid_stft_mag_params": StftMagParams, "aid_matrix_norm_params": MatrixNormParams},
        # (blind.py: aid_stft_band_stats reads x = x_hat, g = |Y| [B, F, T], frames = scratch [B, T, 2, F], out = stats [B, 2, F], adjoint = 0;
        #  aid_lowpass_fit reads den = stats, y = float table [NC cut-offs | NA slopes | floor_dB, k_lo], r = tap window [K], writes g = taps [B, K] and
        #  norm = fit [B, 4]; diag = null, T = NC, ord = NA, max_iter = K, tol = eps)
        launches={"aid_stft_mag": StftMagParams, "aid_matrix_norm_seed": MatrixNormParams,
                  "aid_stft_band_stats": StftMagParams, "aid_lowpass_fit": MatrixNormParams,
                  # (blind_long.py: aid_lowpass_fit's fields, diag = B group ids as ints in HOST memory, read by the launcher)
                  "aid_lowpass_fit_groups": MatrixNormParams}, macros=("AID_LOWPASS_FIT_MAX_ITEMS",)),
    Abi("aid_autoregressive.h", "aid_ar_abi_version", 1,
        structs={"aid_ar_carry_params": ArCarryParams}, launches={"aid_ar_carry": ArCarryParams}),
    Abi("aid_restore.h", "aid_restore_abi_version", 1,
        structs={"aid_window_gather_params": WindowGatherParams, "aid_window_scatter_params": WindowScatterParams},
        launches={"aid_window_gather": WindowGatherParams, "aid_window_scatter": WindowScatterParams, "aid_gap_states": WindowGatherParams},
        macros=("AID_RESTORE_JOB_FIELDS",)),
    Abi("aid_declip.h", "aid_declip_abi_version", 1,
        structs={"aid_clip_known_params": ClipKnownParams, "aid_declip_gather_params": DeclipGatherParams},
        launches={"aid_clip_known": ClipKnownParams, "aid_declip_gather": DeclipGatherParams}),
    Abi("aid_resample_op.h", "aid_resample_op_abi_version", 1,
        structs={"aid_resample_poly_adj_params": ResamplePolyAdjParams}, launches={"aid_resample_poly_adj": ResamplePolyAdjParams}),
    Abi("aid_bwe_long.h", "aid_bwe_long_abi_version", 1,
        structs={"aid_fir_observed_params": FirObservedParams, "aid_bwe_gather_params": BweGatherParams},
        launches={"aid_fir_observed": FirObservedParams, "aid_bwe_gather": BweGatherParams,
                  "aid_iir_observed": FirObservedParams, "aid_iir_gather": BweGatherParams, "aid_fir_clip_observed": FirObservedParams,
                  # (blind.py: aid_fir_observed's fields, h = taps [B, K] with row stride K)
                  "aid_fir_observed_items": FirObservedParams,
                  # (blind_long.py: rec = recordings, jobs = the job table, y = J doubles, the energy of every job's window)
                  "aid_window_energy": BweGatherParams,
                  # (metrics.py: x = estimate, y = reference, state = region weights or null, h = frame distances [B, K], out = 8 doubles per item)
                  "aid_eval_sums": FirObservedParams,
                  # (declick.py: rec = recordings, out = ridge, sigma_floor as 2 floats in HOST memory, y = scores [R, N] with row stride out_ld,
                  #  state = sigma [R, J], L = block, K = order, J = ceil(N / block))
                  "aid_ar_score": BweGatherParams,
                  # (declick.py: x = recordings, y = scores, h = threshold, pad, min_run, max_run as 4 floats in HOST memory, out = mask, mode = 0)
                  "aid_click_mask": FirObservedParams}),
    Abi("aid_lowrate_long.h", "aid_lowrate_long_abi_version", 1,
        structs={"aid_rate_observed_params": RateObservedParams, "aid_lowrate_gather_params": LowrateGatherParams},
        launches={"aid_rate_observed": RateObservedParams, "aid_lowrate_gather": LowrateGatherParams}),
    Abi("aid_phase_long.h", "aid_phase_long_abi_version", 1,
        structs={"aid_stft_mag_observed_params": StftMagObservedParams, "aid_pr_gather_params": PrGatherParams},
        launches={"aid_stft_mag_observed": StftMagObservedParams, "aid_pr_gather": PrGatherParams,
                  # (metrics.py: x = estimate, g = reference, state = region weights or null, frames = k_lo, k_hi, floor as 3 floats in HOST memory,
                  #  out = frame distances [B, T], mode = 0)
                  "aid_stft_logspec_dist": StftMagObservedParams}),
    Abi("aid_spec_long.h", "aid_spec_long_abi_version", 1,
        structs={"aid_stft_mask_observed_params": StftMaskObservedParams, "aid_spec_gather_params": SpecGatherParams},
        launches={"aid_stft_mask_observed": StftMaskObservedParams, "aid_spec_gather": SpecGatherParams}, macros=("AID_SPEC_ITEM_FIELDS",)),
)

_lib = None


def lib():
    """Load libaid_hip.so (built by ``__graft_entry__.build()`` / ``build.py``) and bind every entry of ``ABIS``.  Raises if it is absent, if an export
    is missing or if a header's version is not the one this binding was written against."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise AidError(f"{LIB_PATH} not found: build the HIP extension first (python __graft_entry__.py). "
                           "There is no CPU / eager fallback on the product path.")
        L = C.CDLL(LIB_PATH)
        for abi in ABIS:
            for name in abi.exports:
                if not hasattr(L, name):
                    raise AidError(f"libaid_hip.so does not export {name}")
            for name in abi.launches:
                # (raw addresses, not POINTER(struct): cached launch plans call these with the integer address of a parameter block, see call_on)
                getattr(L, name).restype, getattr(L, name).argtypes = C.c_int, [C.c_void_p, C.c_void_p]
            for name, (restype, argtypes) in {abi.version_fn: (C.c_int, []), **abi.queries}.items():
                getattr(L, name).restype, getattr(L, name).argtypes = restype, argtypes
            if getattr(L, abi.version_fn)() != abi.version:
                raise AidError(f"include/{abi.header} ABI version mismatch")
        _lib = L
    return _lib


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def call(name: str, params) -> None:
    rc = getattr(lib(), name)(C.addressof(params), _stream())
    if rc != 0:
        raise AidError(f"{name} failed rc={rc}: {lib().aid_last_error().decode()}")


def call_on(fn, params_addr: int, stream: int, name: str = "") -> None:
    rc = fn(params_addr, stream)
    if rc != 0:
        raise AidError(f"{name} failed rc={rc}: {lib().aid_last_error().decode()}")


def _req(t: torch.Tensor):
    if not (t.is_cuda and t.dtype == torch.float32):
        raise AidError("HIP kernels need float32 tensors on the GPU (no CPU fallback)")


def ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def view4(t: Optional[torch.Tensor]) -> View:
    """[B,C,F,T] tensor (any strides with T contiguous) -> aid_view."""
    if t is None:
        return View(None, 0, 0, 0)
    _req(t)
    assert t.dim() == 4 and (t.stride(3) == 1 or t.shape[3] == 1), "T must be contiguous"
    return View(t.data_ptr(), t.stride(0), t.stride(1), t.stride(2))


def pack_dims(cin: int, cout: int):
    a, b = C.c_int(0), C.c_int(0)
    lib().aid_conv2d_pack_dims(cin, cout, C.byref(a), C.byref(b))
    return a.value, b.value


def wino8_matrices():
    """(A^T [8,10], G [10,3], B^T [10,10]) of F(8,3) as the kernels use them, float64 (tools/gen_wino8.py writes csrc/aid_wino8.h from the same call)."""
    return winograd.cook_toom(winograd.W8_POINTS, 8, 3)


def wino45_matrices():
    """(AF^T [4,8], GF [8,5], BF^T [8,8], AT^T [4,6], GT [6,3], BT^T [6,6]) of the 2-D form F(4,5) x F(4,3) as the kernels use them, float64
    (tools/gen_wino45.py writes csrc/aid_wino45.h from the same calls)."""
    return winograd.cook_toom(winograd.W45_F_POINTS, 4, 5) + winograd.cook_toom(winograd.W45_T_POINTS, 4, 3)


# The fused 1-D F(4,3) kernels use the classic unscaled matrices over {0, +-1, +-2, inf}, not cook_toom((1, 2), 4, 3) (include/aid_kernels.h, aid_conv2d)
_G43 = torch.tensor([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]],
                    dtype=torch.float64)
_G8, _GF, _GT = (torch.from_numpy(g) for g in (wino8_matrices()[1], wino45_matrices()[1], wino45_matrices()[4]))
# Weight packs of a conv layer by the form number the builder speaks (network._FORMS): (G along kh or None, G along kw or None)
PACK_FORMS = {0: (None, None), 4: (None, _G43), 8: (None, _G8), 45: (_GF, _GT), 85: (_GF, _G8)}


def pack_planes(form: int, kh: int = 5, kw: int = 3) -> int:
    """leading dimension of the pack of a [.., .., kh, kw] weight in this form"""
    gh, gw = PACK_FORMS[form]
    return (kh if gh is None else gh.shape[0]) * (kw if gw is None else gw.shape[0])


def pack_conv_weight_form(w: torch.Tensor, form: int, transpose: bool = False) -> torch.Tensor:
    """[Cout,Cin,KH,KW] (form 0 also [Cout,Cin,k] / [Cout,Cin]) -> the pack [planes, Cin_pad, Cout_pad] (cout contiguous, zero padded) that
    aid_pack_conv_weight writes for this form: U = G_kh w G_kw^T in float64, stored fp32.  Plane order: kh*KW + kw (form 0), xi*5 + kh (1-D forms:
    G along kw only), xf*NT + xt (2-D forms).  transpose=True packs the input-gradient operator instead: taps flipped, roles of Cin/Cout swapped."""
    gh, gw = PACK_FORMS[form]
    if w.dim() == 2:
        w = w[:, :, None, None]
    elif w.dim() == 3:
        w = w[:, :, None, :]  # Conv1d [O,I,k] -> [O,I,1,k]
    w = w.detach().double()
    if transpose:
        w = w.flip(2, 3).permute(1, 0, 2, 3)
    co, ci, kh, kw = w.shape
    assert form == 0 or (kh, kw) == (5, 3)
    if gw is None:
        U = w.permute(2, 3, 1, 0)                                                         # [kh, kw, ci, co]
    elif gh is None and form == 4:
        # (_G43 row by row with each division done once, as aid_pack_conv_weight does it: the device pack is bit-identical)
        w0, w1, w2 = w[..., 0], w[..., 1], w[..., 2]
        U = torch.stack((w0 / 4, -(w0 + w1 + w2) / 6, -(w0 - w1 + w2) / 6, (w0 + 2 * w1 + 4 * w2) / 24,
                         (w0 - 2 * w1 + 4 * w2) / 24, w2), dim=0).permute(0, 3, 2, 1)     # [xi, kh, ci, co]
    elif gh is None:
        U = torch.einsum("xk,oihk->xoih", gw.to(w.device), w).permute(0, 3, 2, 1)         # [xi, kh, ci, co]
    else:
        U = torch.einsum("fh,tk,oihk->ftio", gh.to(w.device), gw.to(w.device), w)         # [xf, xt, ci, co]
    cip, cop = pack_dims(ci, co)
    out = torch.zeros(pack_planes(form, kh, kw), cip, cop, device=w.device, dtype=torch.float32)
    out[:, :ci, :co] = U.reshape(-1, ci, co).float()
    return out


def pack_conv_weight(w: torch.Tensor, transpose: bool = False) -> torch.Tensor:
    return pack_conv_weight_form(w, 0, transpose)


def pack_conv_weight_wino(w: torch.Tensor, transpose: bool = False) -> torch.Tensor:
    return pack_conv_weight_form(w, 4, transpose)


def pack_conv_weight_wino8(w: torch.Tensor, transpose: bool = False) -> torch.Tensor:
    return pack_conv_weight_form(w, 8, transpose)


def pack_conv_weight_wino2d(w: torch.Tensor, transpose: bool = False) -> torch.Tensor:
    return pack_conv_weight_form(w, 45, transpose)


def pack_conv_weight_wino2d8(w: torch.Tensor, transpose: bool = False) -> torch.Tensor:
    return pack_conv_weight_form(w, 85, transpose)


# ---------------------------------------------------------------------------------------------------------
# CQT launch helpers (used by cqt.CQTransform)
# ---------------------------------------------------------------------------------------------------------
def _cqt_params(tr, tab, octs: Sequence[torch.Tensor], window: Optional[torch.Tensor] = None) -> CqtParams:
    P = tr.plan
    p = CqtParams()
    p.tab = CqtTables(P.numocts, P.binsoct, ptr(tab["rc"]), ptr(tab["Lg"]), ptr(tab["goff"]),
                      ptr(tab["g"] if window is None else window), ptr(tab["T_oct"]), ptr(tab["twiddle"]), P.Tmax)
    for o in range(P.numocts):
        p.T_host[o] = int(P.T_oct[o])
        t = octs[o]
        _req(t)
        assert t.shape[1] == 2 and t.shape[2] == P.binsoct and t.shape[3] == P.T_oct[o] and t.stride(3) == 1
        p.oct[o] = View(t.data_ptr(), t.stride(0), t.stride(1), t.stride(2))
    p.B = octs[0].shape[0]
    p.Lh = P.Lh
    p.unnormalized = 0
    return p


def cqt_analysis(tr, tab, spec_ri: torch.Tensor, octs, in_scale=None, window=None, unnormalized=False):
    """spec [B,Lh,2] -> planar octave views.  window=None: analysis windows g (forward transform);
    window=gdM + unnormalized: exact adjoint of synthesis+gather (input-VJP)."""
    _req(spec_ri)
    assert spec_ri.is_contiguous()
    p = _cqt_params(tr, tab, octs, window)
    p.spec = spec_ri.data_ptr()
    p.in_scale = ptr(in_scale)
    p.unnormalized = int(unnormalized)
    call("aid_cqt_analysis", p)


def cqt_synthesis(tr, tab, octs, ws: torch.Tensor):
    p = _cqt_params(tr, tab, octs)
    p.band_ws = ws.data_ptr()
    call("aid_cqt_synthesis", p)


def cqt_gather(tr, tab, ws, Y, X=None, cskip=None, cout=None, hpf=None, window=None, band_scale=None):
    """Y = hpf * (cskip*X + cout * band_scale * sum_k ws_k * window_k).  window=None: dual windows gdM (forward
    synthesis); window = g/T_k: adjoint of the analysis."""
    P = tr.plan
    p = CqtGatherParams(ptr(ws), ptr(tab["kfirst"]), ptr(tab["kcount"]), ptr(tab["rc"]), ptr(tab["Lg"]),
                        ptr(tab["goff"]), ptr(tab["woff"]), ptr(tab["Tk"]), ptr(tab["gdM"] if window is None else window),
                        ptr(X), ptr(cskip), ptr(cout), ptr(hpf), Y.data_ptr(), Y.shape[0], P.Lh, P.ws_per_b, ptr(band_scale))
    call("aid_cqt_gather", p)
