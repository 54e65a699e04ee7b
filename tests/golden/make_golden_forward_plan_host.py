"""Generate tests/golden/forward_plan_host_parent.json: the workspace sizes and refusals of tests/forward_plan_cases.py as the
library gives them BEFORE the forward's host side moved into csrc/lrf_forward.inl.  Recorded once, from a build of that parent
commit (it needs no GPU):

  git worktree add /tmp/parent <parent commit> && (cd /tmp/parent && python __graft_entry__.py)
  python tests/golden/make_golden_forward_plan_host.py /tmp/parent/localrf_amd/csrc/liblrf_hip.so

The library is loaded here, not through localrf_amd._native.lib(): the parent does not export lrf_debug_forward_plan.  A
refusal is kept only if the library returns 1 with a text of its own; anything else (a call that got as far as HIP) is
printed and dropped."""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                         # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))        # the package

import forward_plan_cases as F  # noqa: E402
from localrf_amd import _native as N  # noqa: E402


def load(path):
    h = C.CDLL(path)
    for name, (res, args) in N.SYMBOLS.items():
        fn = getattr(h, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, args
    return h


def main():
    lib = load(sys.argv[1])
    refusals, dropped = {}, []
    for key, (rc, text) in F.refusals(lib).items():
        if rc == 1 and text.startswith(("lrf_", "localrf:")):
            refusals[key] = [rc, text]
        else:
            dropped.append((key, rc, text))
    for d in dropped:
        print("dropped:", d)
    rec = {"sizes": F.sizes(lib), "refusals": refusals}
    path = os.path.join(HERE, "forward_plan_host_parent.json")
    with open(path, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    print(path, os.path.getsize(path), "bytes;", len(rec["sizes"]), "sizes,", len(refusals), "refusals,", len(dropped), "dropped")


if __name__ == "__main__":
    main()
