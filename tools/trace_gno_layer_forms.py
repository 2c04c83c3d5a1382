#!/usr/bin/env python3
"""One GNOConv forward + backward per layer form (the LAYER_CASES of tests/test_gno_forms_gpu.py, each under its own chunk size), for

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o k -- python tools/trace_gno_layer_forms.py [--lib PATH]

: which launches does each form consist of?  --lib runs another build of the library (the parent of a change to the choice of
kernels); `tools/trace_gno_layer_forms.py --names DIR` then prints the library's kernel names of DIR's trace in launch order, so that
two builds' sequences can be compared with diff."""
import argparse
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def names(directory):
    f = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)[0]
    rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))
    for r in rows:
        if "ngpde::" in r["Kernel_Name"]:
            print(r["Kernel_Name"].replace("ngpde::(anonymous namespace)::", "").replace("ngpde::", "").replace("void ", "").split("(")[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None)
    ap.add_argument("--names", default=None, metavar="DIR")
    a = ap.parse_args()
    if a.names:
        return names(a.names)
    import torch
    import ngpde_amd as ng
    from ngpde_amd import _lib
    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)
    import test_gno_forms_gpu as T
    for case in T.LAYER_CASES:
        name, cin, cout, k, aggr, first, b2, N, deg, de, nd, chunk, f_train, f_infer, shape = case
        os.environ["NGPDE_GNO_GFORM_CHUNK"] = str(chunk)
        g, _, ds = T.layer_graph(N, deg, 31, edata=de, node_data=nd, isolated=0 if deg is not None else 3)
        dims, acts = T.phi_dims_acts(shape, 2 * ds + de, k, cin, cout, first)
        phi = ng.Chain(*[ng.Dense(dims[l], dims[l + 1], acts[l], **({"bias": b2} if l + 1 == len(acts) else {})) for l in range(len(acts))])
        layer = ng.GNOConv((cin, cout), phi, "tanh", initialgraph=g, aggr=aggr)
        ps0, st = ng.setup(41, layer)
        ps = T.prep(ps0, 41)
        x = torch.randn(cin, N, device="cuda").requires_grad_(True)
        y, _ = layer(x, ps, st)
        y.sum().backward()
        torch.cuda.synchronize()
        print(name, f_train, flush=True)


if __name__ == "__main__":
    main()
