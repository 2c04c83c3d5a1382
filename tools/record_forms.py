#!/usr/bin/env python3
"""Record a kernel family's golden answers -- its support queries and workspace sizes, as a given build answers them.

    python tools/record_forms.py --family gno|gcn_gat --lib PATH/libngpde_hip.so --commit <hash of the build> [--out FILE]

It asks the questions of the family's float64 test (query_answers there: the same grid, settings and handles) of the library at
--lib, so the file and the test that reads it cannot drift apart.  Needs the GPU for the graph handles; launches no kernel of the
family.  Record from the build BEFORE a change to the choice of kernels, then require equality after it."""
import argparse
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

# family -> (test module with query_answers, golden file, what the file holds)
FAMILIES = {
    "gno": ("test_gno_forms_gpu", "gno_forms.json",
            "ngpde_gno_apply_supported, _message_supported, _gform_supported, _gform_preferred, _gform_splits over the boundary grid and "
            "ngpde_gno_layer_workspace_bytes [inference, training] of the layer cases of tests/test_gno_forms_gpu.py, per switch setting; "
            "the encoding: query_answers there"),
    "gcn_gat": ("test_gcn_forms_gpu", "gcn_gat_forms.json",
                "ngpde_gat_layer_supported, ngpde_node_gat_supported, ngpde_gcn_workspace_bytes [forward, backward], "
                "ngpde_gcn_backward_ew_workspace_bytes, ngpde_gat_workspace_bytes and ngpde_gat_layer_workspace_bytes over the width and "
                "head grids of tests/gcn_gat_forms_spec.py on the handles of tests/test_gcn_forms_gpu.py, per switch setting; the "
                "encoding: setting_answers there"),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--family", required=True, choices=sorted(FAMILIES))
    ap.add_argument("--lib", required=True)
    ap.add_argument("--commit", required=True)
    ap.add_argument("--out")
    args = ap.parse_args()
    module, golden, what = FAMILIES[args.family]
    out = args.out or os.path.join(ROOT, "tests", "golden", golden)
    import importlib
    import pytest
    from ngpde_amd import _lib
    _lib.LIB_PATH = os.path.abspath(args.lib)
    T = importlib.import_module(module)
    with pytest.MonkeyPatch.context() as mp:
        answers = T.query_answers(mp)
    doc = {"recorded_from": args.commit, "what": what}
    doc.update(answers)
    text = re.sub(r"\[\s+(\d+),\s+(\d+)\s+\]", r"[\1, \2]", json.dumps(doc, indent=1))   # a size pair on one line
    text = re.sub(r"(\d,)\n\s+(?=\d)", r"\1 ", text)                                      # a longer list of sizes too
    with open(out, "w") as f:
        f.write(text + "\n")
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
