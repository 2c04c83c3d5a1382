"""csrc/gcn_forms.h and csrc/gat_forms.h against their restatement (tests/gcn_gat_forms_spec.py), with no GPU: every decision of the
GCNConv and GATConv families -- a layer's kind, spmm instantiation, split, column-sum stages and workspace sizes, the fused launches'
template arguments, grids, slabs and guards, the GAT primitives' forms, the one-launch layer's support, grids and workspace, the host
half of the resident solver's support -- over the boundary values of every condition the headers test.

Every form computes the same numbers, so a threshold that drifts in the library passes every float64 comparison: it merely runs a
slower kernel, or stops testing the one a case was written for.  Here the headers' own functions are printed by a stand-alone program
(tests/host/gcn_gat_forms_check.cpp: it includes the two headers alone and is built by the host compiler with
-fsanitize=address,undefined) and every line must equal what the restatement says: once with no switch set, once per switch with that
switch alone.  Each switch must change a decision of the case list, and with no switch set the kernel-name sequences seen must
include every form (REQUIRED below), so that the case list cannot lose a branch unnoticed.  Where the two disagree, the library's
behaviour before the headers existed decides which one is corrected: tests/golden/gcn_gat_forms.json holds its answers, and
test_the_restatement_gives_the_recorded_answers holds the restatement to them here, on the CPU."""
import itertools
import json
import os
import shutil
import subprocess

import pytest

import gcn_gat_forms_spec as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTINGS = [None] + [(name, "1") for name in S.SWITCHES]
ACTS = tuple(S.ACT.values())
NS = (0, 1, 32, 33, 64, 65, 512, 513)


def row_limit(d):
    """the first node count whose rows of d floats reach 2^32 bytes"""
    return S.ROW_BYTES_LIMIT // (4 * d)


def geoms(ns, edges=(0, 1)):
    """every combination of the four bits a choice reads, at each node and edge count"""
    return [S.geom(n, e, ht, hs, norm, loops) for n in ns for e in edges for ht in (0, 1) for hs in (0, 1) for norm in (0, 1) for loops in (0, 1)]


def line(fn, g, *args):
    fields = [int(g[k]) for k in ("graph", "has_norm", "halo_ok", "halo_ok_s", "self_loops", "n_nodes", "n_edges")]
    return fn + " " + " ".join(map(str, fields + [int(a) for a in args]))


def names(ks):
    return ",".join(ks) if ks else "-"


def want_fused_fwd(g, d, act, pre, own):
    f = S.fused_fwd_form(g, d, act, pre, own)
    return (f"supported={int(f['supported'])} rows_ok={int(f['rows_ok'])} pre_ok={int(f['pre_ok'])} launch={int(f['launch'])} act={f['act']} halo={int(f['halo'])} "
            f"pre={int(f['pre'])} own_first={int(f['own_first'])} grid={f['grid']} block={f['block']} {names(S.fused_fwd_names(f))}")


def want_fused_bwd(g, d, act, agg, pre):
    f = S.fused_bwd_form(g, d, act, agg, pre)
    return (f"supported={int(f['supported'])} rows_ok={int(f['rows_ok'])} pre_ok={int(f['pre_ok'])} launch={int(f['launch'])} act={f['act']} halo={int(f['halo'])} "
            f"pair={int(f['pair'])} pre={int(f['pre'])} grid={f['grid']} block={f['block']} slabs={f['slabs']} {names(S.fused_bwd_names(f))}")


def want_fused_sizes(n, d):
    return f"blocks={S.fused_num_blocks(n)} slabs={S.n_slabs(n, d)} mask_bytes={S.fused_mask_bytes(n, d)}"


def want_layer(g, din, dout, act):
    f = S.layer_form(g, din, dout, act)
    ws = ",".join(str(S.layer_workspace_bytes(g, din, dout, b, ew)) for b, ew in ((False, False), (True, False), (True, True)))
    return (f"kind={f['kind']} dp={f['dp']} nsplit={f['nsplit']} parts={f['parts']} colsum_two={int(f['colsum_two_stage'])} "
            f"needs_saved_agg={int(f['needs_saved_agg'])} needs_x={int(f['needs_x'])} ws={ws} fwd={names(S.layer_fwd_names(f))} "
            f"bwd={names(S.layer_bwd_names(f))} bwd_dw_only={names(S.layer_bwd_names(f, dx=False, dbias=False))}")


def want_gat_fwd(g, heads, c):
    return (f"form={S.fwd_form(g, heads, c)} tiled_supported={int(bool(S.gat_tiled_supported(g, heads, c)))} launch={int(g['n_nodes'] > 0)} "
            f"{names(S.fwd_names(g, heads, c))}")


def want_gat_bwd(g, heads, c, aligned):
    return f"form={S.bwd_form(heads, c, aligned)} launch={int(g['n_nodes'] > 0)} ws={S.gat_workspace_bytes(g, heads)} {names(S.bwd_names(g, heads, c, aligned))}"


def want_gat_layer(g, din, heads, c):
    f = S.gat_layer_form(g, din, heads, c)
    fwd, bwd = S.gat_layer_names(f)
    return (f"supported={int(bool(f['supported']))} node={int(bool(S.node_host_supported(g, heads, c)))} h={f['h']} n_tiles={f['n_tiles']} src_wgs={f['src_wgs']} "
            f"ws={S.gat_layer_workspace_bytes(g, heads) if g['graph'] else 0} fwd={names(fwd)} bwd={names(bwd)}")


def all_cases():
    """(line for the program, function that gives the restatement's answer under the environment of the moment)"""
    out = []
    add = lambda fn, want, g, *a: out.append((line(fn, g, *a), lambda: want(g, *a)))
    relu, tanh = S.ACT["relu"], S.ACT["tanh"]
    fits = S.geom(513, 1)
    # the fused launches: every width with every activation; every geometry bit with PRE, own-first tables and the dx launch; the
    # node counts around a tile, a pair and the 2^32-byte guard
    for d in S.WIDTHS:
        for act in ACTS:
            add("fused_fwd", want_fused_fwd, fits, d, act, 0, 0)
            add("fused_bwd", want_fused_bwd, fits, d, act, 1, 0)
    for d in S.FUSED:
        for g in geoms((0, 33)) + [S.geom(n) for n in NS + (row_limit(d) - 1, row_limit(d))] + [S.geom(65, graph=False)]:
            for pre, x, act in itertools.product((0, 1), (0, 1), (relu, S.ACT["identity"], tanh)):
                add("fused_fwd", want_fused_fwd, g, d, act, pre, x)
                add("fused_bwd", want_fused_bwd, g, d, act, x, pre)
            out.append((line("prescaled", g, d), lambda g=g, d=d: f"prescaled={int(bool(S.fused_prescaled_supported(g, d)))}"))
        for n in NS + (row_limit(d),):
            out.append((f"fused_sizes {n} {d}", lambda n=n, d=d: want_fused_sizes(n, d)))
    # a layer: every pair of widths on both sides of the column sum's two stages and of the Dense split; the fused kind's names read
    # the geometry and the activation
    for n in (0, 91, 512, 513, 1241):
        for din, dout in itertools.product(S.WIDTHS + (300, 1433), S.WIDTHS):
            add("layer", want_layer, S.geom(n), din, dout, relu)
    for g in geoms((33,), (1,)):
        for act in ACTS:
            add("layer", want_layer, g, 64, 64, act)
    # the GAT primitives and the layer: every (heads, c) of the grid on every geometry bit; the guard at 64-float rows
    hc = [(h, c) for h in S.HEADS for c in S.head_widths(h)]
    for g in geoms((0, 33)) + [S.geom(n) for n in (row_limit(64) - 1, row_limit(64))] + [S.geom(65, graph=False)]:
        for h, c in hc:
            add("gat_fwd", want_gat_fwd, g, h, c)
            add("gat_layer", want_gat_layer, g, 64, h, c)
            for aligned in (0, 1):
                add("gat_bwd", want_gat_bwd, g, h, c, aligned)
    for din in S.WIDTHS:
        for h, c in hc:
            add("gat_layer", want_gat_layer, fits, din, h, c)
    return out


# what a run without switches must show: each fused forward and pullback instantiation class, the three spmm-first orders at every
# DP with both column sums and the summed split, every GAT primitive form at every <H>, the layer at every <H>
REQUIRED = ({f"gcn_fused_fwd_kernel<{d},{a},{hp}>" for d in S.FUSED for a in ("relu", "identity", "runtime") for hp in ("true,true", "true,false", "false,false")}
            | {f"gcn_fused_bwd_kernel<{d},{ahp[0]},{a},{ahp[1]},{S.tf(d <= 64)},{ahp[2]}>" for d in S.FUSED for a in ("relu", "runtime")
               for ahp in (("true", "true", "true"), ("true", "true", "false"), ("true", "false", "false"), ("false", "false", "true"), ("false", "false", "false"))}
            | {f"spmm_generic_kernel<{dp}>,ngpde_dense_forward" for dp in (8, 16, 32, 64)}
            | {f"dense_forward_split,spmm_generic_kernel<{dp}>" for dp in (8, 16, 32, 64)}
            | {"dense_forward_split,sum_partials_kernel,spmm_generic_kernel<8>",
               "act_bwd_kernel,colsum_kernel,spmm_generic_kernel<16>,dense_backward_weight,dense_backward_input",
               "act_bwd_kernel,colsum_partial_kernel,colsum_kernel,spmm_generic_kernel<16>,dense_backward_weight,dense_backward_input",
               "act_bwd_kernel,dense_backward_weight,dense_backward_input,spmm_generic_kernel<32>", "act_bwd_kernel,dense_backward_weight",
               "zero_bytes_kernel,gcn_fused_bwd_kernel<64,false,relu,false,true,false>,gcn_fused_bwd_kernel<64,true,relu,true,true,false>,reduce_slabs_kernel,reduce_slabs_kernel",
               "zero_bytes_kernel,gcn_fused_bwd_kernel<64,false,relu,false,true,false>,reduce_slabs_kernel", "-"}
            | {"gat_fused_fwd_kernel", "gat_fwd_kernel", "gat_bwd_target_kernel,gat_bwd_source_kernel,gat_scores_bwd_dwx_kernel,gat_scores_bwd_da_kernel"}
            | {f"gat_fwd_blocked_kernel<{h}>" for h in (1, 2, 4, 8, 16)}
            | {f"gat_bwd_target_blocked_kernel<{h}>,gat_bwd_source_blocked_kernel<{h}>,gat_scores_bwd_dwx_kernel,gat_scores_bwd_da_kernel" for h in (1, 2, 4, 8, 16)}
            | {f"gat_layer_fwd_kernel<{h}>" for h in (1, 2, 4)}
            | {f"gat_layer_bwd_target_kernel<{h}>,gat_layer_bwd_source_kernel<{h}>,gat_layer_reduce_kernel" for h in (1, 2, 4)})


def sequences(got):
    """every kernel-name sequence of a run's answers"""
    seen = set()
    for g in got:
        toks = g.split(" ")
        for tok in toks:
            if tok.startswith(("fwd=", "bwd=", "bwd_dw_only=")):
                seen.add(tok.split("=", 1)[1])
        if "=" not in toks[-1] or toks[-1].startswith(("gcn_", "gat_")):
            seen.add(toks[-1])
    return seen


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("gcn_gat_forms") / "gcn_gat_forms_check")
    src = os.path.join(ROOT, "tests", "host", "gcn_gat_forms_check.cpp")
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
    return run(program, [l for l, _ in cases], None)


@pytest.mark.parametrize("setting", SETTINGS, ids=["none"] + ["=".join(s) for s in SETTINGS[1:]])
def test_the_headers_decide_what_the_restatement_says(program, cases, unswitched, setting, monkeypatch):
    for name in S.SWITCHES:                                            # the restatement reads the environment, as the library does
        monkeypatch.delenv(name, raising=False)
    if setting:
        monkeypatch.setenv(*setting)
    got = run(program, [l for l, _ in cases], setting) if setting else unswitched
    wrong = [(l, g, w()) for (l, w), g in zip(cases, got) if g != w()]
    assert not wrong, f"{len(wrong)} of {len(cases)} decisions differ (case, header, restatement): {wrong[:5]}"
    if setting is None:
        seen = sequences(got)
        assert REQUIRED <= seen, sorted(REQUIRED - seen)
        kinds = {g.split(" ")[0] for (l, _), g in zip(cases, got) if l.startswith("layer ")}
        assert kinds == {"kind=fused", "kind=aggregate_first", "kind=multiply_first"}
        parts = {tok for g in got for tok in g.split(" ") if tok.startswith("parts=")}
        assert {"parts=1", "parts=4"} <= parts and len(parts) >= 4
    else:
        changed = {l.split(" ")[0] for (l, _), g, u in zip(cases, got, unswitched) if g != u}
        assert changed == {S.NO_HALO: {"fused_fwd", "fused_bwd", "prescaled", "layer"}, S.NO_FUSED_GAT: {"gat_fwd"}, S.NO_FUSED_GAT_LAYER: {"gat_layer"},
                           S.NO_PERSISTENT: {"gat_layer"}}[setting[0]], setting


def test_the_asymmetries_the_headers_keep(monkeypatch):
    # the tiled primitive needs the normalisation but no edge, the layer needs an edge; each reads its own switch and neither
    # reads NGPDE_NO_HALO; the pre-scaled form needs self loops, the plain staged gather does not
    for name in S.SWITCHES:
        monkeypatch.delenv(name, raising=False)
    g = S.geom(100, 0)
    assert S.fwd_form(g, 4, 16) == "tiled" and not S.layer_supported(g, 64, 4, 16) and S.layer_supported(S.geom(100, 1), 64, 4, 16)
    assert S.fwd_form(S.geom(100, 1, has_norm=False), 4, 16) == "blocked"
    assert S.fused_fwd_form(S.geom(100, self_loops=False), 64, 1, False, False)["halo"] and not S.fused_prescaled_supported(S.geom(100, self_loops=False), 64)
    g = S.geom(100, 1)
    monkeypatch.setenv(S.NO_FUSED_GAT, "0")                            # on when set at all
    assert S.fwd_form(g, 4, 16) == "blocked" and S.layer_supported(g, 64, 4, 16)
    monkeypatch.delenv(S.NO_FUSED_GAT)
    monkeypatch.setenv(S.NO_FUSED_GAT_LAYER, "0")                      # on when 1
    assert S.layer_supported(g, 64, 4, 16)
    monkeypatch.setenv(S.NO_FUSED_GAT_LAYER, "1")
    assert S.fwd_form(g, 4, 16) == "tiled" and not S.layer_supported(g, 64, 4, 16) and not S.node_host_supported(g, 4, 16)
    monkeypatch.delenv(S.NO_FUSED_GAT_LAYER)
    monkeypatch.setenv(S.NO_HALO, "1")
    assert S.fwd_form(g, 4, 16) == "tiled" and S.layer_supported(g, 64, 4, 16) and not S.fused_fwd_form(g, 64, 1, False, False)["halo"]


def test_the_restatement_gives_the_recorded_answers(monkeypatch):
    # tests/golden/gcn_gat_forms.json: what the library answered before the headers existed, on handles whose geometry the file
    # records.  The sizes and the layer's support follow from that geometry alone, so the restatement must reproduce them here; the
    # solver's support also asks the device and may only be narrower than its host half
    doc = json.load(open(os.path.join(ROOT, "tests", "golden", "gcn_gat_forms.json")))["queries"]
    hc = [(h, c) for h in S.HEADS for c in S.head_widths(h)]
    bits = lambda text, count: [b == "1" for group in text.split(" ") for b in bin(int(group, 16))[2:].zfill(4 * len(group))[:count]]
    for setting, per in doc.items():
        for name in S.SWITCHES:
            monkeypatch.delenv(name, raising=False)
        if setting:
            monkeypatch.setenv(*setting.split("="))
        for handle, tables in per.items():
            tables = {q: (doc[""][handle][q] if t == "as unswitched" else t) for q, t in tables.items()}
            n, E, ht, hs = tables["geometry"]
            g = S.geom(n, E, bool(ht), bool(hs))
            what = (setting, handle)
            want = [S.layer_workspace_bytes(g, din, dout, b, ew) for din in S.WIDTHS for dout in S.WIDTHS for b, ew in ((False, False), (True, False), (True, True))]
            assert tables["gcn_workspace_bytes"] == want, what
            assert tables["gat_workspace_bytes"] == [S.gat_workspace_bytes(g, h) for h in S.HEADS], what
            assert tables["gat_layer_workspace_bytes"] == [S.gat_layer_workspace_bytes(g, h) for h in S.HEADS], what
            assert bits(tables["gat_layer_supported"], len(hc)) == [bool(S.layer_supported(g, din, h, c)) for din in S.WIDTHS for h, c in hc], what
            node = bits(tables["node_gat_supported"], len(hc))
            assert all(bool(S.node_host_supported(g, h, c)) or not b for b, (h, c) in zip(node, hc)), what
