"""csrc/dense_forms.h against its restatement (tests/dense_forms_spec.py), with no GPU: every decision of the Dense family -- the
forward form, the backward plan, pair forward, chain forward, pair backward, the chunk / split counts and the workspace size -- over
the boundary values of every condition the header tests.

Every form of a Dense call computes the same numbers, so a threshold that drifts in the library passes every float64 comparison: it
merely runs a slower kernel, or stops testing the one a case was written for.  Here the header's own functions are printed by a
stand-alone program (tests/host/dense_forms_check.cpp: it includes dense_forms.h alone and is built by the host compiler with
-fsanitize=address,undefined) and every line must equal what the restatement says: once with no Dense switch set, once per Dense
switch with that switch alone.  With no switch set the kernel-name sequences seen must include every form (REQUIRED below), so that
the case list cannot lose a branch unnoticed.  Addresses are integers that nobody dereferences.  Where the two disagree, the library's
behaviour before the header existed decides which one is corrected."""
import itertools
import os
import shutil
import subprocess

import pytest

import dense_forms_spec as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = S.ONCE_NAMES + S.PER_CALL

BASE = 0x7F0000000000                      # 256-byte aligned; block b lives at X[b], a misaligned copy 4 bytes further
X = [BASE + (b << 32) for b in range(4)]
WT, Y, Z, DY, WS = (BASE + (k << 32) for k in range(4, 9))
DX = [BASE + (b << 32) for b in range(9, 13)]
OFF = 4                                    # one float: a base that is not 16-byte aligned

# row counts: the bounds of the small forms (65 536), of the streaming pullbacks (32 768, 2^24), the 512-tile thresholds at both tile
# shapes (128 x 64: 511 / 512 row tiles and, at two column tiles, 255 / 256; 128 x 128 at 16 column tiles: 31 / 32), the streaming
# pullback's slab bound at din = 128 (n / 129 = 255 / 256), the weight pullback's one chunk (64) and its % 16 rule (4096 / 4100),
# the split input pullback's 256-tile bound at one column tile (255 / 256 row tiles)
ROWS = (0, 1, 64, 65, 1000, 1024, 3968, 3969, 4096, 4100, 32640, 32641, 32767, 32768, 33023, 33024, 65408, 65409, 65536, 65537,
        2 ** 24, 2 ** 24 + 1)


class Tab:
    """a block table: widths, row_divs and per-block byte offsets of the base from the aligned address"""

    def __init__(self, widths, rds=None, shifts=None, base=None):
        self.widths, self.rds = tuple(widths), tuple(rds or (1,) * len(widths))
        self.shifts = tuple(shifts or (0,) * len(widths))
        self.ptrs = tuple((base or X)[b] + sh for b, sh in zip(range(len(widths)), self.shifts))

    @property
    def T(self):
        return S.table(self.ptrs, self.widths, self.rds)

    def text(self):
        return " ".join([str(len(self.widths))] + [f"{p} {w} {r}" for p, w, r in zip(self.ptrs, self.widths, self.rds)])


NO_TAB = "0"


def case_line(entry, n, a, b=None, d1=0, d2=0, identity=1, bias=0, wt=WT, y=Y, z=Z, dy=DY, ws=WS, dseg=(0, 0, 0, 0)):
    dseg = tuple(dseg) + (0,) * (4 - len(dseg))
    return f"{entry} {n} {a.text()} {b.text() if b else NO_TAB} {d1} {d2} {identity} {bias} {wt} {y} {z} {dy} {ws} " + " ".join(map(str, dseg))


def opt(present, v):
    return str(v) if present else "-"


def names(ks):
    return ",".join(ks) if ks else "-"


# ---- the cases: (line for the program, function of `once` that gives the restatement's answer) -----------------------------------

FWD_TABLES = (
    [Tab((d,)) for d in (16, 17, 32, 48, 64, 65, 128)]
    + [Tab((64,), shifts=(OFF,)), Tab((64,), rds=(2,)), Tab((16,), shifts=(OFF,))]          # vec fails by base address; row_div 2
    + [Tab((2, 64)), Tab((30, 34)), Tab((32, 32, 2)), Tab((32, 32, 2), shifts=(0, OFF, 0))]  # vec fails by offset, by width, by base
    + [Tab((64, 8)), Tab((64, 9)), Tab((96, 8)), Tab((96, 9)), Tab((72, 8)), Tab((72, 9)), Tab((100, 4)), Tab((60, 4, 4)), Tab((40, 3, 5)),
       Tab((64, 3, 5), rds=(1, 1, 700)), Tab((64, 4, 4), rds=(1, 1, 999)), Tab((64, 4, 5))])
FWD_DOUTS = (1, 64, 65, 127, 128, 132, 2048)


def fwd_cases():
    for tab, dout, n in itertools.product(FWD_TABLES, FWD_DOUTS, ROWS):
        variants = [dict()]
        if len(tab.widths) == 1:                                       # the gemm128 operands, misaligned in turn
            variants += [dict(wt=WT + OFF), dict(y=Y + OFF), dict(z=Z + OFF), dict(z=0)]
        for v in variants:
            wt, y, z = v.get("wt", WT), v.get("y", Y), v.get("z", Z)

            def want(once, tab=tab, dout=dout, n=n, wt=wt, y=y, z=z):
                form = S.fwd_form(n, tab.T, dout, wt, y, z, once)
                wide = form in ("dense_stream64_fwd_kernel", "dense_wide_fwd_kernel")
                small = form == "dense_small_fwd_kernel"
                return (f"{form or '-'} din_main={opt(wide, S.din_main(tab.T))} "
                        f"grid={opt(small, S.small_fwd_grid(n, S.din_of(tab.T), dout, once))}")
            yield case_line("fwd", n, tab, d1=dout, wt=wt, y=y, z=z), want


# (table, gradient requests): True = an aligned buffer, OFF = a misaligned one, None = NULL
BWD_TABLES = (
    [(Tab((d,)), g) for d in (1, 16, 17, 64, 65, 128, 130, 132) for g in ((True,), (None,))]
    + [(Tab((64,)), (OFF,)), (Tab((128,)), (OFF,)), (Tab((64,), shifts=(OFF,)), (True,)), (Tab((128,), shifts=(OFF,)), (True,)),
       (Tab((64,), rds=(2,)), (True,)), (Tab((128,), rds=(2,)), (True,))]
    + [(Tab((64, 64)), (True, True)), (Tab((64, 64)), (True, None)), (Tab((64, 64)), (True, OFF)), (Tab((64, 64), rds=(1, 2)), (True, True)),
       (Tab((64, 64, 64)), (True, True, True)), (Tab((64, 64, 2), rds=(1, 1, 9000)), (True, True, True)), (Tab((64, 64, 4)), (True, True, None)),
       (Tab((64, 64, 5)), (True, True, None)), (Tab((2, 64)), (None, True)), (Tab((64, 2)), (True, True)), (Tab((64, 4)), (True, None)),
       (Tab((64, 5)), (True, None)), (Tab((64, 1, 1, 2), rds=(1, 1, 3, 1)), (True, None, None, None)), (Tab((64, 2, 2, 1)), (True, None, None, None)),
       (Tab((33, 31)), (True, None)), (Tab((7, 3, 10), rds=(1, 4, 1)), (True, True, None)), (Tab((40, 60)), (True, True)), (Tab((40, 60)), None)])
BWD_DOUTS = (1, 64, 65, 127, 128, 256, 512, 1024, 2048)


def bwd_cases():
    for (tab, grads), dout, n in itertools.product(BWD_TABLES, BWD_DOUTS, ROWS):
        dseg = [0 if not g else DX[b] + (OFF if g == OFF else 0) for b, g in enumerate(grads)] if grads else None
        variants = [dict(identity=i, bias=b) for i in (0, 1) for b in (0, 1)]
        if len(tab.widths) == 1 and tab.widths[0] >= 128:               # the gemm128 operands, misaligned in turn: dz (= dy under the
            for i in (0, 1):                                           # identity, else the workspace's first piece), weight, partials
                variants += [dict(identity=i, bias=0, dy=DY + OFF), dict(identity=i, bias=0, wt=WT + OFF), dict(identity=i, bias=0, ws=WS + OFF)]
        for v in variants:
            identity, bias = v["identity"], v["bias"]
            wt, dy, ws = v.get("wt", WT), v.get("dy", DY), v.get("ws", WS)

            def want(once, tab=tab, dseg=dseg, dout=dout, n=n, identity=identity, bias=bias, wt=wt, dy=dy, ws=ws):
                T, din = tab.T, S.din_of(tab.T)
                ks = S.bwd_form(n, T, dout, "identity" if identity else "relu", wt, dy, dseg, bool(bias), ws, once)
                grid, n_main = S.stream_bwd_grid(n, T, dout, dseg)
                stream, small = bool(ks) and ks[0].startswith("dense_stream64_bwd"), bool(ks) and ks[0] == "dense_small_bwd_kernel"
                composed = bool(ks) and not stream and not small
                if small:
                    grid = S.small_bwd_grid(n, din, dout, once)
                grads_given = any(bool(dseg and dseg[i]) and s.rd == 1 for i, s in enumerate(T))
                split = grads_given and len(T) == 1 and S.input_splits(n, din, dout) > 1
                _, oper, nz = S.input_split_shape(n, din, dout) if split else (1, dout, 1)
                inp = composed and grads_given
                return (f"{names(ks)} grid={opt(stream or small, grid)} n_main={opt(stream, n_main)} "
                        f"nchunk={opt(composed, S.weight_chunks(n, din, dout))} rpc={opt(composed, S.rows_per_chunk(n, din, dout))} "
                        f"oper={opt(inp, oper)} nz={opt(inp, nz)} workspace={S.workspace_bytes(n, din, dout)}")
            yield case_line("bwd", n, tab, d1=dout, identity=identity, bias=bias, wt=wt, dy=dy, ws=ws, dseg=dseg or ()), want


PAIR_A = (Tab((64,)), Tab((64, 4)), Tab((64, 5)), Tab((64, 2, 2), rds=(1, 1, 1000)), Tab((64,), shifts=(OFF,)), Tab((64,), rds=(2,)),
          Tab((32, 32)), Tab((64, 64)))
PAIR_B = (Tab((64,)), Tab((64, 4)), Tab((64, 5)), Tab((64,), shifts=(OFF,)), Tab((64, 1), base=X[1:]))   # the last: another leading block
PAIR_ROWS = (0, 1, 32767, 32768, 65408, 65409, 2 ** 24, 2 ** 24 + 1)
CHAIN_TABLES = PAIR_A + (Tab((64, 64, 4)), Tab((64, 64, 5)), Tab((64, 64, 64)), Tab((64, 64), shifts=(0, OFF)))


def pair_and_chain_cases():
    for a, b, n in itertools.product(PAIR_A, PAIR_B, PAIR_ROWS):
        for da, db in ((64, 64), (64, 65), (65, 40), (40, 1)):
            def want(once, a=a, b=b, n=n, da=da, db=db):
                fused = bool(S.pair_fwd_fused(n, a.T, da, b.T, db))
                return f"{'dense_pair_fwd_kernel' if fused else '-'} fused={int(fused)}"
            yield case_line("pair_fwd", n, a, b, d1=da, d2=db), want
        for dout in (64, 65):
            def want(once, a=a, b=b, n=n, dout=dout):
                grid = S.pair_bwd_grid(n, a.T, b.T, dout)
                ks = ("dense_pair64_bwd_kernel", "dense_weight_reduce_kernel", "dense_weight_reduce_kernel") if grid else ()
                return f"{names(ks)} grid={grid} workspace={S.pair_bwd_workspace(grid, S.din_of(a.T), S.din_of(b.T))}"
            yield case_line("pair_bwd", n, a, b, d1=dout), want
    for t, n, dmid, dout in itertools.product(CHAIN_TABLES, PAIR_ROWS, (64, 32, 65), (64, 65, 1)):
        def want(once, t=t, n=n, dmid=dmid, dout=dout):
            nm = S.stream_main_blocks(t.T) if S.chain2_fused(n, t.T, dmid, dout) else 0
            return f"{f'dense_chain_fwd_kernel<{nm}>' if nm else '-'} n_main={nm}"
        yield case_line("chain", n, t, d1=dmid, d2=dout), want


def all_cases():
    return list(itertools.chain(fwd_cases(), bwd_cases(), pair_and_chain_cases()))


# what a run without switches must show: every forward kernel and "no launch", both streaming pullbacks, the small one, both weight
# forms, all five outcomes of the input pullback, dense_dz_kernel present and absent, pair forward fused and not, the chain over one,
# two and no block, a pair pullback with and without a grid
REQUIRED = {
    "fwd": {"-", "dense_small_fwd_kernel", "dense_gemm128_fwd_kernel", "dense_stream64_fwd_kernel", "dense_wide_fwd_kernel", "dense_mfma_fwd_kernel"},
    "bwd": {"-", "dense_stream64_bwd_kernel<1>,dense_weight_reduce_kernel", "dense_stream64_bwd_kernel<2>,dense_weight_reduce_kernel",
            "dense_small_bwd_kernel,dense_weight_reduce_kernel",
            "dense_dz_kernel,dense_mfma_bwd_weight_kernel,dense_weight_reduce_kernel",                                  # no input pullback
            "dense_gemm128_split_kernel<true,false>,dense_weight_reduce_kernel,dense_gemm128_split_kernel<false,true>,add_partials_kernel",
            "dense_mfma_bwd_weight_kernel,dense_weight_reduce_kernel,dense_wide_bwd_input_kernel,add_partials_kernel",   # split, 128-row tiles
            "dense_mfma_bwd_weight_kernel,dense_weight_reduce_kernel,dense_wide_bwd_input_kernel",
            "dense_dz_kernel,dense_gemm128_split_kernel<true,false>,dense_weight_reduce_kernel,dense_mfma_bwd_input_kernel"},
    "pair_fwd": {"dense_pair_fwd_kernel fused=1", "- fused=0"},
    "chain": {"dense_chain_fwd_kernel<1> n_main=1", "dense_chain_fwd_kernel<2> n_main=2", "- n_main=0"},
    "pair_bwd": {"dense_pair64_bwd_kernel,dense_weight_reduce_kernel,dense_weight_reduce_kernel grid=512", "- grid=0"},
}


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("dense_forms") / "dense_forms_check")
    src = os.path.join(ROOT, "tests", "host", "dense_forms_check.cpp")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "neuralgraphpde.jl_amd", "csrc"), src, "-o", exe])
    return exe


@pytest.fixture(scope="module")
def cases():
    return all_cases()


def run(program, cases, switch):
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    if switch:
        env[switch] = "1"
    out = subprocess.run([program], input="\n".join(line for line, _ in cases) + "\n", capture_output=True, text=True, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    got = out.stdout.splitlines()
    assert len(got) == len(cases)
    return got


@pytest.fixture(scope="module")
def unswitched(program, cases):
    return run(program, cases, None)


@pytest.mark.parametrize("switch", (None,) + SWITCHES)
def test_the_header_decides_what_the_restatement_says(program, cases, unswitched, switch, monkeypatch):
    for name in SWITCHES:                                              # the per-call switches: the restatement reads the environment
        monkeypatch.delenv(name, raising=False)
    if switch in S.PER_CALL:
        monkeypatch.setenv(switch, "1")
    once = {name: name == switch for name in S.ONCE_NAMES}
    got = run(program, cases, switch) if switch else unswitched
    wrong = [(line, g, want(once)) for (line, want), g in zip(cases, got) if g != want(once)]
    assert not wrong, f"{len(wrong)} of {len(cases)} decisions differ (case, header, restatement): {wrong[:5]}"
    if switch is None:
        seen = {}
        for (line, _), g in zip(cases, got):
            entry = line.split(" ", 1)[0]
            seen.setdefault(entry, set()).add(g if entry in ("pair_fwd", "chain") else g.split(" ")[0] if entry != "pair_bwd"
                                              else " ".join(g.split(" ")[:2]))
        for entry, need in REQUIRED.items():
            assert need <= seen[entry], (entry, sorted(need - seen[entry]))
        # the counts: one and several chunks and splits, with one and several ranges of the outputs
        bwd = [dict(f.split("=") for f in g.split(" ")[1:]) for (line, _), g in zip(cases, got) if line.startswith("bwd ")]
        assert {"1", "2", "1024"} <= {b["nchunk"] for b in bwd} and {"1", "2", "8"} <= {b["nz"] for b in bwd}
        assert {b["grid"] for b in bwd} >= {"1", "256", "512", "1024"}
    else:
        assert got != unswitched, f"{switch} changes no decision of the case list"
