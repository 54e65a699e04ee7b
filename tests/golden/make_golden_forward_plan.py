"""Generate tests/golden/forward_plan_parent.json: util.tensor_digest of every output of the cases of
tests/test_gpu_forward_plan.py, as the library gives them BEFORE the forward's launch shapes moved into one plan
(csrc/lrf_forward.inl).  Recorded once, on the MI355X, from a build of that parent commit:

  git worktree add /tmp/parent <parent commit> && (cd /tmp/parent && python __graft_entry__.py)
  LRF_LIB=/tmp/parent/localrf_amd/csrc/liblrf_hip.so python tests/golden/make_golden_forward_plan.py [out.json]

Every case is rendered twice, and a case whose two runs differ is refused: nothing is written then."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                         # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))        # the package

import test_gpu_forward_plan as T  # noqa: E402
from localrf_amd import _native as N  # noqa: E402


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
    N.lib()
    fields = T.make_fields()
    rec, unstable = {}, []
    for case in T.CASES:
        a, b = T.run_case(fields, case), T.run_case(fields, case)
        differ = sorted(k for k in a if a[k] != b[k])
        if differ:
            unstable.append((T.case_id(case), differ))
        rec[T.case_id(case)] = a
        print(T.case_id(case), len(a), "outputs", "UNSTABLE " + str(differ) if differ else "", flush=True)
    if unstable:
        sys.exit(f"not recorded: {len(unstable)} cases differ between two runs: {unstable}")
    with open(path, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    print(path, os.path.getsize(path), "bytes;", len(rec), "cases from", N.LIB_PATH)


if __name__ == "__main__":
    main()
