"""csrc/gno_forms.h against its restatement (tests/gno_forms_spec.py), with no GPU: every decision of the GNOConv family -- which apply
kernel runs and what the apply and message entries accept, the by-target form's support, preference, chunk, act1 instantiation and
split, and a layer's form bits with the kernel names of its message part -- over the boundary values of every condition the header
tests.

Every form computes the same numbers, so a threshold that drifts in the library passes every float64 comparison: it merely runs a
slower kernel, or stops testing the one a case was written for.  Here the header's own functions are printed by a stand-alone program
(tests/host/gno_forms_check.cpp: it includes gno_forms.h alone and is built by the host compiler with -fsanitize=address,undefined)
and every line must equal what the restatement says: once with no switch set, once per switch with that switch alone
(NGPDE_GNO_GFORM_CHUNK as 16, 32 and 7).  With no switch set the kernel-name sequences seen must include every form (REQUIRED below),
so that the case list cannot lose a branch unnoticed; 16-edge chunks exist only under NGPDE_GNO_GFORM_CHUNK=16 and are required there.
Where the two disagree, the library's behaviour before the header existed decides which one is corrected
(tests/golden/gno_forms.json holds its answers)."""
import itertools
import os
import shutil
import subprocess

import pytest

import gno_forms_spec as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTINGS = [None] + [(name, "1") for name in S.PATH_SWITCHES] + [(S.GNO_GFORM_CHUNK, v) for v in ("16", "32", "7")]
SAME_AS_UNSWITCHED = {(S.GNO_GFORM_CHUNK, "32"), (S.GNO_GFORM_CHUNK, "7")}     # any value but 16 means the default chunk

OUTS = (0, 1, 4, 15, 16, 17, 112, 128, 129, 144, 240, 256, 257, 272)
KS = (0, 1, 8, 15, 16, 17, 32, 33, 48, 64, 65, 128, 256, 257)
INS = (0, 16, 32, 48, 64, 96, 128, 256)
NS = (0, 1, 127, 128, 129, 4096, 1 << 20, (1 << 23) - 1, 1 << 23, 1 << 24)
ACTS = tuple(S.ACT.values())
AGGRS = tuple(S.AGGR.values())


def edge_counts(N):
    return (0, 1, 64 * N - 1, 64 * N, 1 << 30)


def want_apply(out, k):
    f = S.apply_form(out, k)
    return (f"kind={f['kind']} apply_entry={int(f['apply_entry'])} message_entry={int(f['message_entry'])} fwd={names(S.apply_fwd_names(f))} "
            f"bwd={names(S.apply_bwd_names(f))} msg_fwd={names(S.apply_fwd_names(f, True)) if f['message_entry'] else '-'} "
            f"msg_bwd={names(S.apply_bwd_names(f, True)) if f['message_entry'] else '-'} kp_log2={f.get('kp_log2', 0)} rows_per_thread={f.get('rows_per_thread', 0)} nob={f.get('nob', 0)} "
            f"lds_fwd={f.get('lds_fwd', 0)} lds_bwd={f.get('lds_bwd', 0)}")


def want_gform(N, E, cin, k, out, act1, training):
    f = S.gform_form(N, E, cin, k, out, act1, bool(training))
    return (f"supported={int(f['supported'])} rows_ok={int(f['rows_ok'])} preferred={int(f['preferred'])} chunk={f['chunk']} act1={f['act1']} "
            f"nsplit={f['nsplit']} {names(S.gform_names(f))}")


def want_layer(N, E, cin, out, layers, k, act1, last, b2, aggr, training):
    f = S.layer_form(N, E, cin, out, layers, k, act1, last, b2, aggr, bool(training))
    return (f"reassoc={int(f['reassoc'])} has_b2={int(f['has_b2'])} fused_msg={int(f['fused_msg'])} fused_agg={int(f['fused_agg'])} gform={int(f['gform'])} "
            f"n_mid={f['n_mid']} nsplit={f['nsplit']} fwd={names(S.layer_fwd_names(f))} bwd={names(S.layer_bwd_names(f))}")


def names(ks):
    return ",".join(ks) if ks else "-"


def all_cases():
    """(line for the program, function that gives the restatement's answer under the environment of the moment)"""
    relu, ident = S.ACT["relu"], S.ACT["identity"]
    apply_args = list(itertools.product(OUTS, KS))
    gform_args = [(N, E, cin, 64, 128, relu, tr) for N in NS for E in edge_counts(N) for cin in INS for tr in (0, 1)]
    gform_args += [(4096, 64 * 4096, cin, k, out, relu, tr) for cin in (32, 48) for k in KS for out in OUTS for tr in (0, 1)]
    gform_args += [(129, 64 * 129, cin, 64, 48, a, 0) for cin in INS for a in ACTS]
    layer_args = []
    for tr in (0, 1):
        # every (out, k) under every depth of phi; then the graph's counts and `in`; then what the caller passes
        layer_args += [(4096, 64 * 4096, 64, out, L, k, relu, ident, 1, 0, tr) for out in OUTS for k in KS for L in (1, 2, 3)]
        layer_args += [(N, E, cin, 128, 2, 64, relu, ident, 1, 1, tr) for N in NS for E in edge_counts(N) for cin in INS]
        layer_args += [(300, 64 * 300 - tr, 32, out, L, k, a1, last, b2, aggr, tr) for (out, k) in ((128, 64), (256, 64), (48, 48), (129, 64), (144, 16), (16, 32))
                       for L in (1, 2, 3) for a1 in ACTS for last in (ident, relu) for b2 in (0, 1) for aggr in AGGRS]
    out = [(f"apply {o} {k}", lambda o=o, k=k: want_apply(o, k)) for o, k in apply_args]
    out += [("gform " + " ".join(map(str, a)), lambda a=a: want_gform(*a)) for a in gform_args]
    out += [("layer " + " ".join(map(str, a)), lambda a=a: want_layer(*a)) for a in layer_args]
    return out


# what a run without switches must show: the VALU apply pair, the matrix-pipe apply at each k and both NOB (from a given message
# gradient and from the node gradient), the fused message at each k, the by-target form at each `in` for each act1 class, the literal
# contraction, and the reassociated primitives with a middle layer
REQUIRED = ({"gno_apply_fwd_kernel", "gno_apply_bwd_kernel", "-"}
            | {f"gno_apply_mfma_fwd_kernel<{k},{f}>" for k in S.MFMA_K for f in ("true", "false")}
            | {f"gno_apply_mfma_bwd_kernel<{k},{nob},{n}>" for k in S.MFMA_K for nob in (8, 16) for n in ("true", "false")}
            | {f"gno_gform_fwd_kernel<{cin},32,{a}>,dense_gemm128_split_nn_kernel,gno_gform_finish_kernel" for cin in S.GFORM_IN
               for a in ("relu", "identity", "runtime")}
            | {"ngpde_edge_combine_forward,gno_contract_fwd_kernel", "ngpde_edge_combine_forward,ngpde_dense_forward,ngpde_dense_forward,gno_contract_fwd_kernel",
               "ngpde_edge_combine_forward,ngpde_dense_forward,gno_apply_fwd_kernel", "ngpde_edge_combine_forward,ngpde_dense_forward,gno_apply_mfma_fwd_kernel<64,false>",
               "ngpde_segment_reduce_backward,gno_contract_bwd_kernel,ngpde_edge_combine_backward",
               "ngpde_segment_reduce_backward,gno_apply_bwd_kernel,ngpde_dense_backward,ngpde_edge_combine_backward",
               "ngpde_segment_reduce_backward,gno_apply_mfma_bwd_kernel<64,8,false>,ngpde_edge_combine_backward"})
REQUIRED_CHUNK16 = {f"gno_gform_fwd_kernel<{cin},16,{a}>,dense_gemm128_split_nn_kernel,gno_gform_finish_kernel" for cin in S.GFORM_IN
                    for a in ("relu", "identity", "runtime")}


def sequences(got):
    """every kernel-name sequence of a run's answers"""
    seen = set()
    for g in got:
        for tok in g.split(" "):
            if tok.startswith(("fwd=", "bwd=", "msg_fwd=", "msg_bwd=")):
                seen.add(tok.split("=", 1)[1])
        if g.startswith("supported="):
            seen.add(g.rsplit(" ", 1)[1])
    return seen


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("gno_forms") / "gno_forms_check")
    src = os.path.join(ROOT, "tests", "host", "gno_forms_check.cpp")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "neuralgraphpde.jl_amd", "csrc"), src, "-o", exe])
    return exe


@pytest.fixture(scope="module")
def cases():
    return all_cases()


def run(program, lines, setting):
    env = {k: v for k, v in os.environ.items() if k not in S.SWITCHES}
    if setting:
        env[setting[0]] = setting[1]
    out = subprocess.run([program], input="\n".join(lines) + "\n", capture_output=True, text=True, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    got = out.stdout.splitlines()
    assert len(got) == len(lines)
    return got


@pytest.fixture(scope="module")
def unswitched(program, cases):
    return run(program, [line for line, _ in cases], None)


@pytest.mark.parametrize("setting", SETTINGS, ids=["none"] + ["=".join(s) for s in SETTINGS[1:]])
def test_the_header_decides_what_the_restatement_says(program, cases, unswitched, setting, monkeypatch):
    for name in S.SWITCHES:                                            # the restatement reads the environment, as the library does
        monkeypatch.delenv(name, raising=False)
    if setting:
        monkeypatch.setenv(*setting)
    got = run(program, [line for line, _ in cases], setting) if setting else unswitched
    wrong = [(line, g, w()) for (line, w), g in zip(cases, got) if g != w()]
    assert not wrong, f"{len(wrong)} of {len(cases)} decisions differ (case, header, restatement): {wrong[:5]}"
    if setting is None:
        seen = sequences(got)
        assert REQUIRED <= seen, sorted(REQUIRED - seen)
        nsplit = {tok for g in got for tok in g.split(" ") if tok.startswith("nsplit=")}
        assert {"nsplit=1", "nsplit=8", "nsplit=16", "nsplit=32"} <= nsplit
        bits = {g.split(" n_mid=")[0] for (line, _), g in zip(cases, got) if line.startswith("layer ")}
        assert bits == {f"reassoc={r} has_b2={b} fused_msg={m} fused_agg={a} gform={g}"
                        for r, b, m, a, g in ((0, 0, 0, 0, 0), (1, 0, 0, 0, 0), (1, 1, 0, 0, 0), (1, 0, 1, 0, 0), (1, 1, 1, 0, 0), (1, 0, 1, 1, 0), (1, 1, 1, 1, 0),
                                              (1, 0, 1, 1, 1), (1, 1, 1, 1, 1))}
    elif setting in SAME_AS_UNSWITCHED:
        assert got == unswitched, f"{setting} must leave the default chunk"
    else:
        assert got != unswitched, f"{setting} changes no decision of the case list"
        if setting == (S.GNO_GFORM_CHUNK, "16"):
            assert REQUIRED_CHUNK16 <= sequences(got), sorted(REQUIRED_CHUNK16 - sequences(got))


def test_the_pullback_of_the_matrix_pipe_never_needs_a_raised_lds_limit(program):
    # 32 staged edges x ((64 + 4) z columns + (256 + 4) dm columns) x 4 bytes at the envelope's corner: below the 64 KB a launch may ask
    # for as it is, which is why gno_mfma.hip sets no function attribute (gno_forms.h asserts the same at compile time)
    assert run(program, ["lds_max"], None) == ["max_pullback_lds=41984"]
    assert S.MFMA_BWD_LDS_MAX == 32 * (68 + 260) * 4 == 41984 <= 64 * 1024


def test_the_entries_keep_their_asymmetry(monkeypatch):
    # ngpde_gno_apply_* accept iff the VALU envelope holds, ngpde_gno_message_* iff the matrix-pipe envelope does: 256 x 64 runs on the
    # matrix pipe through the message entries and is refused by the apply entries (tests/test_gno_forms_gpu.py meets both on the device)
    for name in S.SWITCHES:
        monkeypatch.delenv(name, raising=False)
    f = S.apply_form(256, 64)
    assert (f["kind"], f["apply_entry"], f["message_entry"]) == ("mfma", False, True)
    assert all(S.apply_form(out, k)["apply_entry"] == (out * k < 256 * 64) for out in (16, 48, 128, 256) for k in S.MFMA_K)
