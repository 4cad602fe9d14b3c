"""Every environment knob the code reads is listed in the "Env knobs"
section of NOTES.md, and every knob listed there is still read."""

import pathlib
import re

ROOT = pathlib.Path(__file__).resolve().parent.parent
NAME = r"(CYG_[A-Z0-9_]+|CYGAN_[A-Z0-9_]+)"
# getenv("X") in the HIP sources; os.environ.get("X") / os.environ["X"] /
# os.environ.setdefault("X") in Python; _knob_off("X") is ops/conv.py's
# one-line wrapper around os.environ.get
READ = re.compile(
    r"(?:getenv|os\.environ(?:\.\w+)?|_knob_off)\s*[(\[]\s*[\"']" + NAME)


def _knobs_read():
    files = [ROOT / "bench.py", ROOT / "main.py", ROOT / "setup.py"]
    files += [p for p in (ROOT / "cyclegan_amd").rglob("*")
              if p.suffix in (".py", ".hip", ".cpp", ".h")
              and not p.name.endswith("_hip.hip")]  # hipify build copies
    names = set()
    for p in files:
        names.update(READ.findall(p.read_text(errors="replace")))
    return names


def _knobs_documented():
    notes = (ROOT / "NOTES.md").read_text()
    m = re.search(r"^## Env knobs\n(.*?)(?=^## |\Z)", notes, re.S | re.M)
    assert m, "NOTES.md has no '## Env knobs' section"
    return set(re.findall(NAME, m.group(1)))


def test_knobs_documented():
    read, documented = _knobs_read(), _knobs_documented()
    assert len(read) >= 10, f"knob scan found too little: {sorted(read)}"
    assert read - documented == set(), "read but not in NOTES.md"
    assert documented - read == set(), "in NOTES.md but no longer read"
