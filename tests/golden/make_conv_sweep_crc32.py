"""Records tests/golden/conv_sweep_crc32.json (tests/test_gpu_embed_layers.py::test_sweep_bits_are_the_parents) on an MI355X:

    PVF_LIBRARY=<libpvface.so built from the PARENT commit> python tests/golden/make_conv_sweep_crc32.py <that commit's hash>

The library is never the build of the change under test: the fixture says what the code before it wrote."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "pyannote-video_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

if __name__ == "__main__":
    if len(sys.argv) != 2 or not os.environ.get("PVF_LIBRARY"):
        sys.exit(__doc__)
    import test_gpu_embed_layers as T
    from pyannote_video_amd.runtime import Context
    ctx = Context(0)
    out = {"_meta": {"commit": sys.argv[1], "numpy": np.__version__, "device": "MI355X (gfx950)",
                     "what": "zlib.crc32 of debug_conv's output bytes and flag bytes per case of SWEEP, seed 1000 + k"}}
    for split in (False, True):
        out["split" if split else "exact"] = T.sweep_crcs(ctx, split)
    ctx.close()
    with open(os.path.join(ROOT, "tests", "golden", "conv_sweep_crc32.json"), "w") as f:           # one line per case
        f.write('{"_meta": %s,\n' % json.dumps(out["_meta"], sort_keys=True))
        for form in ("exact", "split"):
            rows = ["  %s: %s" % (json.dumps(k), json.dumps(v)) for k, v in sorted(out[form].items())]
            f.write(' "%s": {\n%s\n }%s\n' % (form, ",\n".join(rows), "," if form == "exact" else ""))
        f.write("}\n")
