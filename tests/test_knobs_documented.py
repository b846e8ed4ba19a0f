"""DESIGN.md's "Runtime knobs" table lists exactly the GCSLAM_* environment variables the library
and the Python package read: a knob added or removed without its row fails here.  Its "Build-time
switches" table lists exactly the GCS_* names the sources' preprocessor conditionals test."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "gc-slam_amd")
# getenv("GCSLAM_X") in the C++ / HIP sources; os.environ.get("GCSLAM_X" ...), os.environ["GCSLAM_X"] in Python
READ = re.compile(r'(?:getenv\(|os\.environ(?:\.get\(|\[))\s*"(GCSLAM_[A-Z0-9_]+)"')
ROW = re.compile(r"^\| `(GCSLAM_[A-Z0-9_]+)` \|", re.M)
# #if / #ifdef / #ifndef / #elif lines of the C++ / HIP sources, and the GCS_* names on them
COND = re.compile(r"^[ \t]*#[ \t]*(?:if|ifdef|ifndef|elif)\b(.*)$", re.M)
SWITCH = re.compile(r"\bGCS_[A-Z0-9_]+")
SWITCH_ROW = re.compile(r"^\| `(GCS_[A-Z0-9_]+)` \|", re.M)


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


def _switches_tested():
    names = set()
    csrc = os.path.join(PKG, "csrc")
    for f in os.listdir(csrc):
        if f.endswith((".h", ".hip", ".cpp")):
            with open(os.path.join(csrc, f), encoding="utf-8") as fh:
                for cond in COND.findall(fh.read()):
                    names.update(SWITCH.findall(cond))
    return names


def _switches_documented():
    with open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8") as fh:
        text = fh.read()
    table = text.split("### Build-time switches", 1)[1].split("\n## ", 1)[0]
    return set(SWITCH_ROW.findall(table))


def test_build_time_switch_table_matches_the_code():
    tested, documented = _switches_tested(), _switches_documented()
    # the scan finds something: the patterns still match the sources
    assert tested and "GCS_PHASE_PROF" in tested, sorted(tested)
    assert tested == documented, {"undocumented": sorted(tested - documented), "stale rows": sorted(documented - tested)}
