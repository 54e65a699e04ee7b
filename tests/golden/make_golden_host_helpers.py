"""Generate tests/golden/host_helpers_parent.json: the workspace sizes and refusal texts of tests/host_helpers_cases.py as the
library gives them BEFORE the host helpers moved into csrc/lrf_host.inl.  Recorded once, from a build of that parent commit:

  git worktree add /tmp/parent <parent commit> && (cd /tmp/parent && python __graft_entry__.py)
  LRF_LIB=/tmp/parent/localrf_amd/csrc/liblrf_hip.so python tests/golden/make_golden_host_helpers.py

Runs against this repository's own library only and needs no GPU.  A refusal case is kept only if the recorded library
returns 1 with a text of its own: a case that returns 0, or whose text comes from a HIP call (it then differs between a
machine with and without a device), is dropped and printed; host_helpers_cases.py lists the ones known in advance."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                         # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))        # the package

import host_helpers_cases as H  # noqa: E402
from localrf_amd import _native as N  # noqa: E402


def main():
    lib = N.lib()
    refusals, dropped = {}, []
    for key, (rc, text) in H.refusals(lib).items():
        if rc == 1 and text.startswith(("lrf_", "LrfFrameWindow")):
            refusals[key] = [rc, text]
        else:
            dropped.append((key, rc, text))
    for d in dropped:
        print("dropped:", d)
    rec = {"sizes": H.sizes(lib), "refusals": refusals}
    path = os.path.join(HERE, "host_helpers_parent.json")
    with open(path, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    print(path, os.path.getsize(path), "bytes;", len(rec["sizes"]), "sizes,", len(refusals), "refusals,", len(dropped), "dropped")


if __name__ == "__main__":
    main()
