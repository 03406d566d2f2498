"""Record tests/golden/ws_bytes.json: what every workspace-size query returns over the sweep of tests/ws_bytes_cases.py.  No GPU.
modegpt_amd is imported from PYTHONPATH if it is there (a built checkout of the commit whose sizes are to be pinned), else from this
tree; the sweep always comes from this tree.

    PYTHONPATH=/path/to/built/parent python scripts/record_ws_bytes.py [--out tests/golden/ws_bytes.json]
"""
import argparse
import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(ROOT)                      # (behind PYTHONPATH)

from modegpt_amd import _lib  # noqa: E402

# (by path: the checkout on PYTHONPATH has a `tests` package of its own)
_spec = importlib.util.spec_from_file_location("ws_bytes_cases", os.path.join(ROOT, "tests", "ws_bytes_cases.py"))
ws_bytes_cases = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ws_bytes_cases)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "ws_bytes.json"))
    a = ap.parse_args()
    lib = _lib.load()
    rows = [[fn, list(args), int(getattr(lib, fn)(*args))] for fn, args in ws_bytes_cases.cases()]
    with open(a.out, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")
    print("%d rows from %s -> %s (%d bytes)" % (len(rows), os.path.dirname(_lib.__file__), a.out, os.path.getsize(a.out)))


if __name__ == "__main__":
    main()
