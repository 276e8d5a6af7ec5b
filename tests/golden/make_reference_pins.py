#!/usr/bin/env python
"""Generates tests/golden/reference_pins.json.gz: what the real munkres package and the REFERENCE'S OWN tracking.py,
face/clustering.py and structure/shot.py (executed verbatim through tests/refhost.py) return on the seeded inputs of
tests/test_reference_pins.py, tests/test_reference_clustering.py and tests/test_shot.py (each module's `record`).  The reference
is not part of this repository, so its results travel as this fixture and the tests compare the product and the oracle with it.
    PVF_REFERENCE=<pyannote-video checkout> [PVF_MUNKRES=<munkres.py>] python tests/golden/make_reference_pins.py
"""
import gzip
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "pyannote-video_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import refhost
    if not (refhost.have_reference() and refhost.have_munkres()):
        sys.exit("PVF_REFERENCE must name a pyannote-video checkout and munkres must be importable (or PVF_MUNKRES name its munkres.py)")
    import test_reference_clustering
    import test_reference_pins
    import test_shot
    out = {}
    for mod in (test_reference_pins, test_reference_clustering, test_shot):
        out.update(mod.record())
    with gzip.GzipFile(refhost.PINS, "wb", mtime=0) as f:
        f.write(json.dumps(out, sort_keys=True).encode())
    print(refhost.PINS, os.path.getsize(refhost.PINS), "bytes:", ", ".join("%s %d" % (k, len(v)) for k, v in sorted(out.items())))


if __name__ == "__main__":
    main()
