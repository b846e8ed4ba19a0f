"""DESIGN.md's "Runtime knobs" table lists exactly the GCSLAM_* environment variables the library
and the Python package read: a knob added or removed without its row fails here."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "gc-slam_amd")
# getenv("GCSLAM_X") in the C++ / HIP sources; os.environ.get("GCSLAM_X" ...), os.environ["GCSLAM_X"] in Python
READ = re.compile(r'(?:getenv\(|os\.environ(?:\.get\(|\[))\s*"(GCSLAM_[A-Z0-9_]+)"')
ROW = re.compile(r"^\| `(GCSLAM_[A-Z0-9_]+)` \|", re.M)


def _names_read():
    names = set()
    for sub in ("csrc", "gcslam"):
        for d, _, files in os.walk(os.path.join(PKG, sub)):
            for f in files:
                if f.endswith((".cpp", ".hip", ".h", ".py")):
                    with open(os.path.join(d, f), encoding="utf-8") as fh:
                        names.update(READ.findall(fh.read()))
    return names


def _names_documented():
    with open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8") as fh:
        text = fh.read()
    table = text.split("### Runtime knobs", 1)[1].split("\n## ", 1)[0]
    return set(ROW.findall(table))


def test_runtime_knob_table_matches_the_code():
    read, documented = _names_read(), _names_documented()
    assert len(read) > 20, sorted(read)  # the scan reads something: the patterns still match the sources
    assert read == documented, {"undocumented": sorted(read - documented), "stale rows": sorted(documented - read)}
