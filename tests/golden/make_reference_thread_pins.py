#!/usr/bin/env python
"""Generates tests/golden/reference_thread_pins.json: what the REFERENCE'S OWN structure/thread.py (executed verbatim through
tests/refhost_thread.py, with tests/orb_ref.py behind its cv2) returns for the clip of tests/thread_clip.py -- the threads, the scenes
and the edges of its thread graph with their match counts -- and the pairs its product_lookahead yields for small (n, lookahead).
The GPU test of the `thread` verb and the CPU tests of tests/test_thread.py compare with this file.
    PVF_REFERENCE=<pyannote-video checkout> python tests/golden/make_reference_thread_pins.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "pyannote-video_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

CLIP = {"width": 480, "height": 270, "frames_per_shot": 20, "setups": "ABACBA", "seed": 7}
PINS = os.path.join(HERE, "reference_thread_pins.json")


def main():
    import refhost_thread
    import thread_clip
    if not refhost_thread.have_reference():
        sys.exit("PVF_REFERENCE must name a pyannote-video checkout")
    frames, shots, fps = thread_clip.make_clip(**CLIP)
    threads, scenes, edges = refhost_thread.run_reference(thread_clip.ClipVideo(frames, fps), shots, min_match=20, lookahead=24)
    mod = refhost_thread.reference_thread_module()
    lookahead_pairs = {"%d,%d" % (n, la): sorted(mod.product_lookahead(range(n), la)) for n in range(0, 10) for la in range(1, 8)}
    out = {"product_lookahead": lookahead_pairs, "clip": CLIP, "frame_rate": fps, "shots": shots, "min_match": 20, "lookahead": 24,
           "edges": sorted([i, k, n] for (i, k), n in edges.items()),
           "threads": threads.for_json(), "scenes": scenes.for_json()}
    with open(PINS, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(PINS, os.path.getsize(PINS), "bytes")


if __name__ == "__main__":
    main()
