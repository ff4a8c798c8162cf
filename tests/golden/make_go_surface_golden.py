"""Record the exported surface of the reference's sketches package (every exported func / method with its receiver kind, parameter
and result TYPES; the exported type names; the sentinel errors' names and texts; the fields of IdxValue) into
tests/golden/go_surface.json.  Data only: names and signatures, parsed with the same `surface()` the test applies to the shim.

    python tests/golden/make_go_surface_golden.py <reference checkout>      # the directory that holds sketches/*.go
"""
import glob
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from test_go_shim_surface import surface  # noqa: E402


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    ref = os.path.join(sys.argv[1], "sketches")
    files = sorted(f for f in glob.glob(os.path.join(ref, "*.go")) if not f.endswith("_test.go"))
    assert files, f"no Go sources under {ref}"
    funcs, types, errs, fields = surface(files)
    out = {"source": "sketches/*.go (without *_test.go)",
           "funcs": {k: [v[0], list(v[1]), list(v[2])] for k, v in sorted(funcs.items())},
           "types": sorted(types), "errs": dict(sorted(errs.items())),
           "fields": {k: [list(t) for t in v] for k, v in fields.items()}}
    with open(os.path.join(HERE, "go_surface.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", len(funcs), "funcs,", len(types), "types,", len(errs), "sentinels")


if __name__ == "__main__":
    main()
