#!/usr/bin/env python3
"""Record tests/golden/gno_forms.json: the GNOConv family's query answers and layer workspace sizes, as a given build answers them.

    python tools/record_gno_forms.py --lib PATH/libngpde_hip.so --commit <hash of the build> [--out tests/golden/gno_forms.json]

It asks the questions of tests/test_gno_forms_gpu.py (query_answers: the same grid, settings and layer cases) of the library at --lib,
so the file and the test that reads it cannot drift apart.  Needs the GPU for the layer cases' graph handles; launches no kernel of
the family.  Record from the build BEFORE a change to the choice of kernels, then require equality after it."""
import argparse
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", required=True)
    ap.add_argument("--commit", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "gno_forms.json"))
    args = ap.parse_args()
    import pytest
    from ngpde_amd import _lib
    _lib.LIB_PATH = os.path.abspath(args.lib)
    import test_gno_forms_gpu as T
    with pytest.MonkeyPatch.context() as mp:
        answers = T.query_answers(mp)
    doc = {"recorded_from": args.commit,
           "what": "ngpde_gno_apply_supported, _message_supported, _gform_supported, _gform_preferred, _gform_splits over the boundary grid and "
                   "ngpde_gno_layer_workspace_bytes [inference, training] of the layer cases of tests/test_gno_forms_gpu.py, per switch setting; "
                   "the encoding: query_answers there"}
    doc.update(answers)
    text = re.sub(r"\[\s+(\d+),\s+(\d+)\s+\]", r"[\1, \2]", json.dumps(doc, indent=1))   # a size pair on one line
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
