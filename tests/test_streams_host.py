"""Which entries tests/test_streams_gpu.py runs on a side stream, accounted against include/ngpde.h (no device call: CPU).

Every prototype that carries an ngpde_stream_t is either declared by a case of that module -- which the GPU test then has to reach with
the side stream's handle -- or named in its ALLOW list, which is a condition and not a convenience: at most 8 names, each with a
reason, only collectives that need a communicator and pure diagnostics."""
import os
import re

from ngpde_amd import _lib
import test_streams_gpu as S
from test_abi import header_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIAGNOSTICS = {"ngpde_node_profile", "ngpde_node_pipeline_stats"}


def test_stream_positions_agree_with_the_binding_table():
    assert set(S.STREAM_AT) <= set(header_functions())
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ngpde.h")).read(), flags=re.S)
    assert len(S.STREAM_AT) == len(re.findall(r"ngpde_stream_t\s+\w+\s*[,)]", src))          # one per prototype, none missed
    for name, at in S.STREAM_AT.items():
        types = _lib.SIGNATURES[name][1]
        assert at < len(types) and types[at] is _lib._vp, (name, at)


def test_every_stream_entry_is_declared_by_a_case_or_allowed():
    with_stream = set(S.STREAM_AT)
    declared = set(S.DECLARED) - set(S.CREATES)
    assert declared <= with_stream, sorted(declared - with_stream)
    assert not declared & set(S.ALLOW), sorted(declared & set(S.ALLOW))
    missing = with_stream - declared - set(S.ALLOW)
    assert not missing, f"{len(missing)} entries take a stream and no case declares them: {sorted(missing)}"
    assert set(S.ALLOW) <= with_stream, sorted(set(S.ALLOW) - with_stream)


def test_the_allow_list_is_short_and_holds_collectives_and_diagnostics_only():
    assert len(S.ALLOW) <= 8
    for name, reason in S.ALLOW.items():
        assert isinstance(reason, str) and len(reason.strip()) > 10 and "\n" not in reason, name
        collective = name.startswith("ngpde_grad_allreduce") and _lib.SIGNATURES[name][1][0] is _lib._vp          # (takes the communicator first)
        assert collective or name in DIAGNOSTICS or name.endswith("_fault"), name
        assert not re.search(r"forward|backward|create|build|sample|solve|_cg|query|has_edge", name), name


def test_the_streamless_creates_are_declared_by_a_solver_case():
    for create in ("ngpde_node_vmh_create", "ngpde_ode_create"):
        assert create in _lib.SIGNATURES and create not in S.STREAM_AT
        cases = [name for name, (_, entries, _) in S.CASES.items() if create in entries]
        assert cases and all(name.startswith("solver") for name in cases), (create, cases)


def test_case_names_are_unique_test_ids():
    assert len(S.CASES) == len(set(S.CASES)) and all(entries for _, entries, _ in S.CASES.values())
