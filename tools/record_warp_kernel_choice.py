#!/usr/bin/env python3
"""Record tests/golden/warp_kernel_choice.json: the kernel every case of tests/test_gpu_warp_kernel_choice.py launches.

The table is the yardstick of a change to the warp launchers, so it is recorded in a checkout of the commit BEFORE that change (with
this file and the test module copied into it), on the GPU, and only the JSON is carried over:

    python tools/record_warp_kernel_choice.py [out.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]


def main():
    table_path = os.path.join(ROOT, 'tests', 'golden', 'warp_kernel_choice.json')
    out = sys.argv[1] if len(sys.argv) > 1 else table_path
    if not os.path.exists(table_path):                # (the test module loads the table when it is imported)
        with open(table_path, 'w') as fh:
            fh.write("{}\n")
    import torch
    import test_gpu_warp_kernel_choice as t
    from oflibpytorch_amd import _native
    _native.load_library()
    dev = torch.device('cuda', 0)
    table = {}
    for case in sorted(t.CASES, key=lambda c: (c["n"], c["h"], c["w"], c["id"])):
        table[case["id"]] = t.run_case(case, dev)[1]
    torch.cuda.synchronize()
    with open(out, 'w') as fh:
        json.dump(table, fh, indent=0, sort_keys=True)
        fh.write("\n")
    print("%d cases, %d distinct kernels -> %s" % (len(table), len(set(table.values())), out))


if __name__ == '__main__':
    main()
