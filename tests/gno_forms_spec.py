"""Which kernels a GNOConv call runs, restated in Python line for line from csrc/gno_forms.h: tests/test_gno_forms_host.py compares
this with the header's own functions, and the float64 tests (tests/test_gno_forms_gpu.py) take the form a layer case must show from
here.  The environment is read at every call, as the library reads it."""
import os

# ---- the family's constants ---------------------------------------------------------------------------------------------------------
BATCH, THREADS, MAX_DIM, MAX_ROWS_PER_THREAD, VALU_LDS_LIMIT = 16, 256, 256, 32, 60 * 1024   # VALU apply
ET, EB, EBB = 16, 64, 32                                                                     # matrix pipe: tile, edges per pass fwd / bwd
MFMA_OUT_STEP, MFMA_OUT_MAX, MFMA_K = 16, 256, (16, 32, 64)
NOB_SMALL, NOB_LARGE, NOB_SMALL_MAX_OUT = 8, 16, 128
GK, GFORM_IN = 64, (32, 64, 128)                                                             # by target
CHUNK, CHUNK_ALT = 32, 16
TRAIN_EDGES_PER_NODE = 64
ROW_BYTES_LIMIT = 1 << 32
SPLIT_TILE, SPLIT_TARGET_WGS, SPLIT_MIN_K, SPLIT_CAP = 128, 512, 256, 32

ACT = {"identity": 0, "relu": 1, "tanh": 2, "sigmoid": 3, "swish": 4, "gelu": 5, "leakyrelu": 6, "elu": 7, "softplus": 8}
AGGR = {"+": 0, "mean": 1, "max": 2, "min": 3, "*": 4}

NO_GNO_MFMA, NO_GNO_GFORM, GNO_MATERIALIZE, GNO_GFORM_CHUNK = "NGPDE_NO_GNO_MFMA", "NGPDE_NO_GNO_GFORM", "NGPDE_GNO_MATERIALIZE", "NGPDE_GNO_GFORM_CHUNK"
SWITCHES = (NO_GNO_MFMA, NO_GNO_GFORM, GNO_MATERIALIZE, GNO_GFORM_CHUNK)
PATH_SWITCHES = SWITCHES[:3]


def on(name):
    """a yes/no switch: on when the value starts with 1 (read per call)"""
    return os.environ.get(name, "")[:1] == "1"


def atoi(text):
    """C's atoi: leading blanks, a sign, then digits; 0 where there are none"""
    t = text.lstrip(" \t\n\v\f\r")
    sign, i = 1, 0
    if t[:1] in ("+", "-"):
        sign, i = (-1 if t[0] == "-" else 1), 1
    j = i
    while j < len(t) and t[j].isdigit() and t[j].isascii():
        j += 1
    return sign * int(t[i:j]) if j > i else 0


# ---- the apply kernels ----------------------------------------------------------------------------------------------------------------
def pad4(v):
    return (v + 3) & ~3


def kp_log2(k):
    l = 0
    while (1 << l) < k:
        l += 1
    return l


def rows_per_thread(out, k):
    og = THREADS >> kp_log2(k)
    return pad4((pad4(out) + og - 1) // og)


def valu_lds(out, k, bwd):
    cP, kP = pad4(out), pad4(k)
    return (kP * (cP + 1) + BATCH * kP + (BATCH * cP if bwd else 0)) * 4


def valu_envelope(out, k):
    if out <= 0 or k <= 0 or out > MAX_DIM or k > MAX_DIM:
        return False
    return rows_per_thread(out, k) <= MAX_ROWS_PER_THREAD and valu_lds(out, k, True) <= VALU_LDS_LIMIT


def mfma_shape(out, k):
    return out % MFMA_OUT_STEP == 0 and MFMA_OUT_STEP <= out <= MFMA_OUT_MAX and k in MFMA_K


def mfma_bwd_lds(out, k):
    return (EBB * (k + 4) + EBB * (out + 4)) * 4


MFMA_BWD_LDS_MAX = max(mfma_bwd_lds(o, k) for o in range(MFMA_OUT_STEP, MFMA_OUT_MAX + 1, MFMA_OUT_STEP) for k in MFMA_K)


def mfma_envelope(out, k):
    return not on(NO_GNO_MFMA) and mfma_shape(out, k)


def apply_form(out, k):
    """kind: what the apply launchers run; apply_entry / message_entry: what ngpde_gno_apply_* / ngpde_gno_message_* accept -- the VALU
    envelope and the matrix-pipe envelope, an asymmetry the entries keep (256 x 64: message yes, apply no)"""
    f = {"kind": "unsupported", "apply_entry": valu_envelope(out, k), "message_entry": mfma_envelope(out, k), "k": k}
    if f["message_entry"]:
        f.update(kind="mfma", nob=NOB_SMALL if out <= NOB_SMALL_MAX_OUT else NOB_LARGE, lds_fwd=0, lds_bwd=mfma_bwd_lds(out, k))
    elif f["apply_entry"]:
        f.update(kind="valu", kp_log2=kp_log2(k), rows_per_thread=rows_per_thread(out, k), lds_fwd=valu_lds(out, k, False), lds_bwd=valu_lds(out, k, True))
    return f


def _tf(b):
    return "true" if b else "false"


def apply_fwd_names(f, fused=False):
    if f["kind"] == "unsupported":
        return []
    return ["gno_apply_fwd_kernel"] if f["kind"] == "valu" else [f"gno_apply_mfma_fwd_kernel<{f['k']},{_tf(fused)}>"]


def apply_bwd_names(f, node=False):
    if f["kind"] == "unsupported":
        return []
    return ["gno_apply_bwd_kernel"] if f["kind"] == "valu" else [f"gno_apply_mfma_bwd_kernel<{f['k']},{f['nob']},{_tf(node)}>"]


# ---- the by-target form ---------------------------------------------------------------------------------------------------------------
def gform_supported(cin, k):
    return not on(NO_GNO_GFORM) and k == GK and cin in GFORM_IN


def gform_splits(N, cin, k, out):
    tiles = ((N + SPLIT_TILE - 1) // SPLIT_TILE) * ((out + SPLIT_TILE - 1) // SPLIT_TILE)
    ns = max(1, (SPLIT_TARGET_WGS + tiles - 1) // max(tiles, 1))
    ns = min(ns, max(1, (cin * k) // SPLIT_MIN_K))
    return min(ns, SPLIT_CAP)


def gform_form(N, E, cin, k, out, act1, training):
    f = {"in": cin, "supported": gform_supported(cin, k), "rows_ok": N * max(cin, GK) * 4 < ROW_BYTES_LIMIT}
    f["preferred"] = f["supported"] and out % 4 == 0 and E > 0 and f["rows_ok"] and (not training or E >= TRAIN_EDGES_PER_NODE * N)
    env = os.environ.get(GNO_GFORM_CHUNK)
    f["chunk"] = CHUNK_ALT if env is not None and atoi(env) == CHUNK_ALT else CHUNK
    f["act1"] = "relu" if act1 == ACT["relu"] else "identity" if act1 == ACT["identity"] else "runtime"
    f["nsplit"] = gform_splits(N, cin, k, out)
    return f


def gform_names(f):
    if not f["supported"]:
        return []
    return [f"gno_gform_fwd_kernel<{f['in']},{f['chunk']},{f['act1']}>", "dense_gemm128_split_nn_kernel", "gno_gform_finish_kernel"]


# ---- a layer ----------------------------------------------------------------------------------------------------------------------------
def layer_form(N, E, cin, out, phi_layers, k, act1, last_act, b2, aggr, training):
    f = {"apply": apply_form(out, k)}
    f["reassoc"] = phi_layers >= 2 and last_act == ACT["identity"] and not on(GNO_MATERIALIZE) and f["apply"]["apply_entry"]
    f["has_b2"] = f["reassoc"] and bool(b2)
    f["fused_msg"] = (f["reassoc"] and phi_layers == 2 and E > 0 and act1 in (ACT["identity"], ACT["relu"]) and f["apply"]["message_entry"])
    f["fused_agg"] = f["fused_msg"] and aggr in (AGGR["+"], AGGR["mean"])
    f["by_target"] = gform_form(N, E, cin, k, out, act1, training)
    f["gform"] = f["fused_agg"] and f["by_target"]["preferred"]
    f["n_mid"] = 0 if f["fused_msg"] else (phi_layers - 2 if f["reassoc"] else phi_layers - 1)
    f["nsplit"] = f["by_target"]["nsplit"] if f["gform"] else 1
    return f


def layer_fwd_names(f):
    if f["gform"]:
        return gform_names(f["by_target"])
    if f["fused_msg"]:
        return apply_fwd_names(f["apply"], True)
    ks = ["ngpde_edge_combine_forward"] + ["ngpde_dense_forward"] * max(f["n_mid"], 0)
    return ks + (apply_fwd_names(f["apply"]) if f["reassoc"] else ["gno_contract_fwd_kernel"])


def layer_bwd_names(f):
    if f["fused_agg"]:
        return apply_bwd_names(f["apply"], True)
    ks = ["ngpde_segment_reduce_backward"] + (apply_bwd_names(f["apply"]) if f["reassoc"] else ["gno_contract_bwd_kernel"])
    return ks + ["ngpde_dense_backward"] * max(f["n_mid"], 0) + ["ngpde_edge_combine_backward"]


def layer_form_name(f):
    """the name tests/test_gno_forms_gpu.py gives a layer's form"""
    return "gform" if f["gform"] else "fused-agg" if f["fused_agg"] else "fused-msg" if f["fused_msg"] else "reassoc" if f["reassoc"] else "literal"
