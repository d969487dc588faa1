"""The experiment switches: one table in the library (csrc/sg_switch.h), one in the package (switches.py), and DESIGN.md's appendix
restating both.  Text checks only - nothing here loads the library or touches a GPU."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "building_detection_amd")


def _read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def _files(top, *exts):
    return sorted(p for p in glob.glob(os.path.join(ROOT, top, "**", "*"), recursive=True)
                  if os.path.isfile(p) and p.endswith(exts) and "__pycache__" not in p)


def _library_switches():
    return {"SG_" + n for n in re.findall(r"^\s*X\(([A-Z0-9_]+), (?:FLAG|INT|OFF0|DBL),", _read(os.path.join(PKG, "csrc", "sg_switch.h")), re.M)}


def _package_switches():
    return set(re.findall(r'^    "(SG_[A-Z0-9_]+)": \(', _read(os.path.join(PKG, "switches.py")), re.M))


def _appendix():
    """(names with a row in the two tables, names of the retired list)"""
    text = _read(os.path.join(ROOT, "DESIGN.md"))
    text = text[text.index("## Appendix — experiment switches"):]
    live, retired = text.split("### Retired")
    row = re.compile(r"^\| `(SG_[A-Z0-9_]+)`", re.M)
    return set(row.findall(live)), set(row.findall(retired))


def test_the_library_reads_its_environment_in_one_header():
    hits = [os.path.relpath(p, ROOT) for p in _files("building_detection_amd/csrc", ".hip", ".h") if "getenv(" in _read(p)]
    assert hits == ["building_detection_amd/csrc/sg_switch.h"]


def test_the_package_reads_its_switches_in_one_module():
    hits = [os.path.relpath(p, ROOT) for p in _files("building_detection_amd", ".py")
            if os.path.basename(p) != "switches.py" and re.search(r"environ[^\n]*SG_|getenv[^\n]*SG_", _read(p))]
    assert hits == []


def test_design_appendix_has_exactly_the_rows_of_the_two_tables():
    lib, pkg = _library_switches(), _package_switches()
    assert len(lib) > 30 and len(pkg) >= 16   # the patterns above still find the tables
    live, _ = _appendix()
    assert live == lib | pkg


def test_switch_accessor_keeps_each_truth_rule(monkeypatch):
    import importlib.util
    spec = importlib.util.spec_from_file_location("_switches", os.path.join(PKG, "switches.py"))   # (no package import: no torch, no library)
    sw = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sw)
    for name in sw.SWITCHES:
        monkeypatch.delenv(name, raising=False)
    assert sw.get("SG_BN_ADD") is True and sw.get("SG_BN_PW") is False and sw.get("SG_CONV_NOTHIN") is False
    assert sw.get("SG_SIDE_WGRAD") == 1 and sw.get("SG_JIT_LANE_BLOCKS") == 24 and sw.get("SG_SIDE_KEEP_GIB") == 4.0
    monkeypatch.setenv("SG_BN_ADD", "2")      # eq1: "2" is off
    monkeypatch.setenv("SG_BN_CONV", "2")     # ne0: "2" is on
    monkeypatch.setenv("SG_CONV_NOTHIN", "0")  # flag: set is on
    assert sw.get("SG_BN_ADD") is False and sw.get("SG_BN_CONV") is True and sw.get("SG_CONV_NOTHIN") is True
    monkeypatch.setenv("SG_BN_CONV", "0")     # read again at every call
    assert sw.get("SG_BN_CONV") is False


def test_no_retired_switch_is_left_in_code_tests_or_scripts():
    live, retired = _appendix()
    gone = retired - live   # (a switch that lost only some of its values is still live)
    assert len(gone) >= 7
    pat = re.compile(r"\b(" + "|".join(sorted(gone)) + r")\b")
    hits = [(os.path.relpath(p, ROOT), m.group(1)) for top in ("building_detection_amd", "tests", "scripts")
            for p in _files(top, ".py", ".hip", ".h", ".sh", ".md", ".txt", "Makefile") for m in [pat.search(_read(p))] if m]
    assert hits == []
