"""The Dense family's choice of kernels, restated in Python: the written specification of csrc/dense_forms.h.

Every Dense entry picks its kernel(s) from the shape, the pointers' alignment and tile-count thresholds; the library makes each
choice in one pure function of csrc/dense_forms.h (dense_fwd_plan, dense_bwd_plan, dense_pair_fwd_plan, dense_chain_fwd_plan,
dense_pair_bwd_plan), whose head comment gives the order in which the forms are tried.  This module restates the choices
independently.  tests/test_dense_forms_host.py holds the header to it line by line over the boundary values of every condition
(tests/host/dense_forms_check.cpp prints the header's decisions; no GPU), and tests/test_dense_forms_gpu.py uses it to assert that
each of its float64 cases lands on the kernel it means to test.

ngpde_dense_forward (fwd_form):
  small    dense_small_fwd_kernel       17 <= din <= 64, 1 <= dout <= 64, 1 <= n <= 65 536
  gemm128  dense_gemm128_fwd_kernel     one block, 16-byte loadable (`vec`), row_div 1, din % 16 == 0, dout % 4 == 0, dout >= 128,
                                        ceil(n / 128) * ceil(dout / 128) >= 512 tiles, weight, y and save_z 16-byte aligned
  stream   dense_stream64_fwd_kernel    128-row tiles (ceil(n / 128) * ceil(dout / 64) >= 512), din_main == 64, dout <= 64 and every
                                        block before din_main `vec` and inside it
  wide     dense_wide_fwd_kernel        128-row tiles otherwise
  general  dense_mfma_fwd_kernel        everything else
  din_main: trailing blocks with at most 8 features behind them leave the K loop when their offset is a multiple of 32.
  vec (Seg): offset % 4 == 0, width % 4 == 0 and a 16-byte aligned base.
ngpde_dense_multi_forward: dense_mfma_multi_fwd_kernel over the problems with rows (none: no launch).
ngpde_dense_pair_forward (pair_fwd_fused): dense_pair_fwd_kernel when ceil(n / 128) >= 512 (NGPDE_DENSE_NO_STREAM2 unset), both douts
  <= 64 and both sides are ONE leading 64-wide `vec` row_div-1 block at the same address plus <= 4 narrow features; two forwards
  otherwise.
ngpde_dense_chain2_forward (chain2_fused): dense_chain_fwd_kernel<1 / 2> under the same tile rule when dmid == 64, dout <= 64 and the
  table has one or two leading 64-wide blocks plus <= 4 narrow features; two forwards otherwise, and then a1 is required.
ngpde_dense_backward (bwd_form):
  stream   dense_stream64_bwd_kernel<1 / 2> + reduce   dout == 64, 32 768 <= n <= 2^24, one or two 64-wide row_div-1 aligned blocks
                                        (aligned gradient too), <= 4 other features and none of them with a gradient, grid =
                                        min(ceil(n / 64), 512, n / (din + 1)) >= 256 (stream_bwd_grid; NGPDE_DENSE_NO_STREAM_BWD)
  small    dense_small_bwd_kernel + reduce      din, dout <= 64, n <= 65 536, grid = min(ceil(n / 64), 1024, n / (din + 1)) >= 1
  composed dense_dz_kernel (act != identity); dense_gemm128_split_kernel<true,false> (no dbias, > 1 chunk, one vec block, din and
           dout >= 128 and % 4, n % 16 == 0, dz and slabs aligned) or dense_mfma_bwd_weight_kernel; dense_weight_reduce_kernel; then
           for the input pullback: one block and input_splits > 1 -> dense_gemm128_split_kernel<false,true> (din >= 128,
           din % 4, dout % 16, aligned) or dense_wide_bwd_input_kernel split over z, + add_partials_kernel when split;
           otherwise dense_wide_bwd_input_kernel at 128-row tiles, dense_mfma_bwd_input_kernel below.
ngpde_dense_pair_backward (pair_bwd_grid): dense_pair64_bwd_kernel + two reduces when dout == 64, 32 768 <= n <= 2^24 and both sides
  are one aligned 64-wide leading block at the same address plus <= 4 features; ERR_UNSUPPORTED otherwise.

NGPDE_DENSE_NARROW, _NO_GEMM128, _NO_STREAM, _NO_SMALL_FWD and _NO_SMALL_BWD are read once per process (any value): the functions
that depend on them take them as `once`, a dict of name -> bool, which defaults to ONCE, the process environment at import.
NGPDE_DENSE_NO_STREAM2 and _NO_STREAM_BWD are read per call ("1"), from the environment at the time of the call.
"""
import os

ONCE_NAMES = ("NGPDE_DENSE_NARROW", "NGPDE_DENSE_NO_GEMM128", "NGPDE_DENSE_NO_STREAM", "NGPDE_DENSE_NO_SMALL_FWD", "NGPDE_DENSE_NO_SMALL_BWD")
ONCE = {k: os.environ.get(k) is not None for k in ONCE_NAMES}
PER_CALL = ("NGPDE_DENSE_NO_STREAM2", "NGPDE_DENSE_NO_STREAM_BWD")


def env_on(name):
    v = os.environ.get(name)
    return bool(v) and v[0] == "1"


def cdiv(a, b):
    return -(-a // b)


def align256(b):
    return (b + 255) & ~255


class Seg:
    def __init__(self, ptr, w, rd, off):
        self.ptr, self.w, self.rd, self.off = ptr or 0, w, max(rd, 1), off
        self.vec = off % 4 == 0 and w % 4 == 0 and self.ptr % 16 == 0      # fill_seg_table


def table(ptrs, widths, rds):
    segs, off = [], 0
    for p, w, rd in zip(ptrs, widths, rds):
        segs.append(Seg(p, w, rd, off))
        off += w
    return segs


def din_of(T):
    return sum(s.w for s in T)


def aligned(*ptrs):
    return all((p or 0) % 16 == 0 for p in ptrs)


def small_fwd_grid(n, din, dout, once=None):
    if (once or ONCE)["NGPDE_DENSE_NO_SMALL_FWD"] or not (17 <= din <= 64 and 1 <= dout <= 64 and 1 <= n <= 65536):
        return 0
    return min(cdiv(n, 64), 1024)


def small_bwd_grid(n, din, dout, once=None):
    if (once or ONCE)["NGPDE_DENSE_NO_SMALL_BWD"] or not (1 <= din <= 64 and 1 <= dout <= 64 and 1 <= n <= 65536):
        return 0
    g = min(cdiv(n, 64), 1024, n // (din + 1))
    return g if g >= 1 else 0


def wide_tiles(n, cols, once=None):
    return not (once or ONCE)["NGPDE_DENSE_NARROW"] and cdiv(n, 128) * cdiv(cols, 64) >= 512


def din_main(T):
    din, dm = din_of(T), din_of(T)
    for s in reversed(T[1:]):
        if din - s.off > 8:
            break
        if s.off % 32 == 0:
            dm = s.off
    return dm


def fwd_form(n, T, dout, wt, y, z, once=None):
    """the kernel ngpde_dense_forward launches (None: no launch)"""
    once = once or ONCE
    din = din_of(T)
    if n == 0:
        return None
    if small_fwd_grid(n, din, dout, once):
        return "dense_small_fwd_kernel"
    if (not once["NGPDE_DENSE_NO_GEMM128"] and len(T) == 1 and T[0].vec and T[0].rd == 1 and din % 16 == 0 and dout % 4 == 0
            and dout >= 128 and cdiv(n, 128) * cdiv(dout, 128) >= 512 and aligned(wt, y, z)):
        return "dense_gemm128_fwd_kernel"
    if wide_tiles(n, dout, once):
        dm = din_main(T)
        ok = not once["NGPDE_DENSE_NO_STREAM"] and dm == 64 and dout <= 64
        ok = ok and all(s.vec and s.off + s.w <= dm for s in T if s.off < dm)
        return "dense_stream64_fwd_kernel" if ok else "dense_wide_fwd_kernel"
    return "dense_mfma_fwd_kernel"


def stream2(n):
    return not env_on("NGPDE_DENSE_NO_STREAM2") and cdiv(n, 128) >= 512


def stream_main_blocks(T):
    nm = 0
    while nm < len(T) and T[nm].w == 64 and T[nm].rd == 1 and T[nm].vec:
        nm += 1
    return nm if nm >= 1 and din_of(T) - 64 * nm <= 4 else 0


def pair_fwd_fused(n, Ta, douta, Tb, doutb):
    return (stream2(n) and douta <= 64 and doutb <= 64 and stream_main_blocks(Ta) == 1 and stream_main_blocks(Tb) == 1
            and Ta[0].ptr == Tb[0].ptr)


def chain2_fused(n, T, dmid, dout):
    return 0 < n < 2 ** 31 and stream2(n) and dmid == 64 and dout <= 64 and stream_main_blocks(T) in (1, 2)


def stream_bwd_grid(n, T, dout, dseg):
    if env_on("NGPDE_DENSE_NO_STREAM_BWD") or dout != 64 or n < 32768 or n > 2 ** 24:
        return 0, 0
    n_main = n_narrow = 0
    for i, s in enumerate(T):
        grad = bool(dseg and dseg[i]) and s.rd == 1
        if s.w == 64 and s.rd == 1 and s.ptr % 16 == 0 and (not grad or dseg[i] % 16 == 0):
            n_main += 1
        elif grad:
            return 0, 0
        else:
            n_narrow += s.w
    if not 1 <= n_main <= 2 or n_narrow > 4:
        return 0, 0
    g = min(cdiv(n, 64), 512, n // (din_of(T) + 1))
    return (g, n_main) if g >= 256 else (0, 0)


def weight_chunks(n, din, dout):
    tiles = max(1, cdiv(din, 64)) * max(1, cdiv(dout, 64))
    return max(1, min(1024, cdiv(4096, tiles), cdiv(n, 64)))


def input_splits(n, din, dout):
    tiles = cdiv(n, 128) * cdiv(din, 64)
    if tiles == 0 or tiles >= 256 or dout < 512:
        return 1
    return max(1, min(cdiv(2048, tiles), dout // 256))


def workspace_bytes(n, din, dout):
    ns = input_splits(n, din, dout)
    split = (ns - 1) * n * din * 4 if ns > 1 else 0
    return align256(max(n, 1) * dout * 4) + align256(weight_chunks(n, din, dout) * (din + 1) * dout * 4) + align256(split) + 256


def input_split_shape(n, din, dout):
    """(splits, outputs per range, ranges) of the split input pullback"""
    ns = input_splits(n, din, dout)
    oper = cdiv(cdiv(dout, ns), 32) * 32
    return ns, oper, cdiv(dout, oper)


def rows_per_chunk(n, din, dout):
    """rows of one slab of the composed weight pullback"""
    return max(16, cdiv(cdiv(n, weight_chunks(n, din, dout)), 16) * 16)


def bwd_form(n, T, dout, act, wt, dy, dseg, has_bias, ws, once=None):
    """the kernels ngpde_dense_backward launches, in order (() for n == 0: two fills)"""
    once = once or ONCE
    din = din_of(T)
    if n == 0:
        return ()
    g, nm = stream_bwd_grid(n, T, dout, dseg)
    if g:
        return (f"dense_stream64_bwd_kernel<{nm}>", "dense_weight_reduce_kernel")
    if small_bwd_grid(n, din, dout, once):
        return ("dense_small_bwd_kernel", "dense_weight_reduce_kernel")
    ks = []
    dz = dy if act == "identity" else ws
    if act != "identity":
        ks.append("dense_dz_kernel")
    partial = ws + align256(n * dout * 4)
    nchunk = weight_chunks(n, din, dout)
    if (not once["NGPDE_DENSE_NO_GEMM128"] and not has_bias and nchunk > 1 and len(T) == 1 and T[0].vec and T[0].rd == 1
            and din >= 128 and din % 4 == 0 and dout >= 128 and dout % 4 == 0 and n % 16 == 0 and n < 2 ** 30 and aligned(dz, partial)):
        ks.append("dense_gemm128_split_kernel<true,false>")
    else:
        ks.append("dense_mfma_bwd_weight_kernel")
    ks.append("dense_weight_reduce_kernel")
    grads = [bool(dseg and dseg[i]) and s.rd == 1 for i, s in enumerate(T)]
    if any(grads) and len(T) == 1 and input_splits(n, din, dout) > 1:
        _, oper, nz = input_split_shape(n, din, dout)
        part = partial + align256(nchunk * (din + 1) * dout * 4)
        if (not once["NGPDE_DENSE_NO_GEMM128"] and nz > 1 and din >= 128 and din % 4 == 0 and dout % 16 == 0 and oper % 16 == 0
                and n < 2 ** 30 and aligned(dz, wt, dseg[0], part)):
            ks += ["dense_gemm128_split_kernel<false,true>", "add_partials_kernel"]
        else:
            ks += ["dense_wide_bwd_input_kernel"] + (["add_partials_kernel"] if nz > 1 else [])
    elif any(grads):
        ks.append("dense_wide_bwd_input_kernel" if wide_tiles(n, din, once) else "dense_mfma_bwd_input_kernel")
    return tuple(ks)


def pair_bwd_grid(n, Ta, Tb, dout):
    def side_ok(T):
        return len(T) >= 1 and T[0].w == 64 and T[0].rd == 1 and T[0].ptr % 16 == 0 and din_of(T) - 64 <= 4
    if dout != 64 or env_on("NGPDE_DENSE_NO_STREAM_BWD") or n < 32768 or n > 2 ** 24:
        return 0
    if not side_ok(Ta) or not side_ok(Tb) or Ta[0].ptr != Tb[0].ptr:
        return 0
    return min(cdiv(n, 64), 512)


def pair_bwd_workspace(grid, dina, dinb):
    return grid * (dina + dinb + 2) * 64 * 4 + 512 if grid else 0
