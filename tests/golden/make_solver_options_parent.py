"""Records tests/golden/solver_options_parent.jsonl: every sequence of tests/solver_options_cases.entries() driven through the
library that ZF_LIB_PATH names, in a fresh process, on an MI355X -

    ZF_LIB_PATH=<libzfista_hip.so built from the parent commit> python tests/golden/make_solver_options_parent.py "<parent commit>" OUT.jsonl

One JSON line per entry: [group, base, initialised, calls, [plan at creation, [return code, plan] per call]].  The committed file
was recorded from the commit its first line names; tests/test_gpu_solver_options.py replays it against the library of the tree, and
tests/test_solver_options_cpp.py its return codes against csrc/zf_solver_options.h without a device.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main(parent, out_path):
    import solver_options_cases as S

    assert os.environ.get("ZF_LIB_PATH"), "ZF_LIB_PATH must name the library to record"
    drv = S.Driver()
    with open(out_path, "w") as f:
        f.write(json.dumps({"parent": parent, "abi": int(drv.lib.zf_abi_version())}) + "\n")
        for group, base, init, calls in S.entries():
            f.write(json.dumps([group, base, init, calls, drv.run(base, init, calls)], separators=(",", ":")) + "\n")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
