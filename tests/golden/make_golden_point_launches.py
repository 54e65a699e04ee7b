"""Generate tests/golden/point_layer_launches.json: the launch sequences of tests/point_layer_cases.py as the point-side Python
layer made them BEFORE its checks, device step and batcher were shared (cloud.py, mesh_distance.py and alignment.py each with
their own chunk loops).  Recorded once, on an MI355X, from a checkout of that parent commit with this file and
tests/point_layer_cases.py copied in (they use public names only, so they run there unchanged):

  python tests/golden/make_golden_point_launches.py [output path]

The file holds symbol names and small integers only."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                         # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))        # the package

import point_layer_cases  # noqa: E402


def main():
    rec = point_layer_cases.launch_lists()
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "point_layer_launches.json")
    with open(path, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    print(path, os.path.getsize(path), "bytes;", len(rec), "calls,", sum(len(v) for v in rec.values()), "launches")


if __name__ == "__main__":
    main()
