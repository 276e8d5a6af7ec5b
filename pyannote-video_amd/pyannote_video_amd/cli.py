"""`pyannote-face` verbs on the HIP path (reference scripts/pyannote-face.py:29-89 usage, :239-314 bodies, :415-455 dispatch).

    python -m pyannote_video_amd track   [options] <video> <shot.json> <tracking>
    python -m pyannote_video_amd extract [options] <video> <tracking> <landmark_model> <embedding_model> <landmarks> <embeddings>
    python -m pyannote_video_amd cluster [options] <embeddings> <labels>
    python -m pyannote_video_amd process [options] <video> <shot.json> <landmark_model> <embedding_model> <tracking> <landmarks> <embeddings>
    python -m pyannote_video_amd shot    [options] <video> <output.json>
    python -m pyannote_video_amd thread  [--min-match 20] [--lookahead 24] <video> <shot.json> <output.json>
    python -m pyannote_video_amd scene   <video> <thread.json> <output.json>
    python -m pyannote_video_amd storyboard [--per 1] [--width 160] [--columns C] [--thread PATH] [--by time|thread] [--from 0] [--until T]
                                         [--index PATH] [--batch 64] <video> <shot.json> <output>
    python -m pyannote_video_amd enroll  [--append] <video> <landmark_model> <embedding_model> <name> <gallery>
    python -m pyannote_video_amd enroll-track [--append] <embeddings> <track> <name> <gallery>
    python -m pyannote_video_amd identify [--threshold 0.6] [--metric euclidean|cosine] [--labels PATH] [--unknown NAME] [--scores PATH] <embeddings> <gallery> <output>
    python -m pyannote_video_amd search  [-k 100] [--max-distance D] [--rows] [--include-self] (--gallery PATH --name NAME | --from EMBEDDINGS --track ID)
                                         <output> <embeddings> [<embeddings> ...]
    python -m pyannote_video_amd cast    [-k 64] [--max-distance 0.6] [--threshold 2.0] [--by track|face] [--labels SUFFIX] [--graph PATH]
                                         <output> <embeddings> [<embeddings> ...]
    python -m pyannote_video_amd demo    [--height 400] [--from 0] [--until T] [--shift 0] [--landmark PATH] [--label PATH] <video> <tracking> <output>
    python -m pyannote_video_amd redact  [--height 0] [--from 0] [--until T] [--shift 0] [--label PATH] [--only A,B | --keep A,B] [--pad 25] [--cells 8]
                                         [--shape ellipse|box] [--mode mosaic|smooth|fill] [--colour r,g,b] [--draw] <video> <tracking> <output>
    python -m pyannote_video_amd faces   [--per 4] [--tile 150] [--columns C] [--label PATH] [--only A,B] [--spread 1.0] [--min-size 0]
                                         [--max-dark 0.25] [--max-bright 0.25] [--from 0] [--until T] [--index PATH] [--quality PATH]
                                         <video> <tracking> <landmarks> <output>
    python -m pyannote_video_amd talk    [--window 0.4] [--on 3.0] [--off 1.5] [--min-duration 0.3] [--max-pause 0.3] [--max-dark 0.25]
                                         [--from 0] [--until T] [--label PATH] [--segments PATH] <video> <tracking> <landmarks> <output>
    python -m pyannote_video_amd fingerprint [--from 0] [--until T] [--batch 64] <video> <prints.npy>
    python -m pyannote_video_amd repeat  [--max-bits 10] [--flat 16] [--min-duration 2.0] [--max-gap 0.5] [--min-separation 5.0]
                                         <output.json> <prints.npy> [<prints.npy> ...]
    python -m pyannote_video_amd blend   [--width 64] [--from 0] [--until T] [--batch 64] <video> <blend.npy>
    python -m pyannote_video_amd transition [--move 4.0] [--linear 0.25] [--flat 2.0] [--min-duration 0.12] [--shots IN --refined OUT]
                                         [--motion motion.npy] <blend.npy> <output.json>
    python -m pyannote_video_amd motion  [--width 96] [--from 0] [--until T] [--batch 256] <video> <motion.npy>
    python -m pyannote_video_amd camera  [--pan 5] [--zoom 3] [--window 0.5] [--min-inliers 50] [--min-duration 0.5] [--max-gap 0.2]
                                         [--shots shot.json] <motion.npy> <output.json>
    python -m pyannote_video_amd text    [--step 0] [--edge 48] [--still 8] [--on 24] [--from 0] [--until T] [--batch 64] <video> <text.npy>
    python -m pyannote_video_amd caption [--window 1.0] [--hold 0.5] [--gap 1] [--min-duration 1.0] [--min-width 3] [--max-height 0.25]
                                         [--fill 0.5] [--rows 0,1] [--tracking PATH] <text.npy> <output.json>
    python -m pyannote_video_amd clothes [--widen 0.5] [--drop 0.25] [--height 2.0] [--bands 2] [--min-size 0] [--keep-overlapped]
                                         [--from 0] [--until T] [--batch 2048] <video> <tracking> <clothes.npy>
    python -m pyannote_video_amd link    [--min-score 0.75] [--margin 0.05] [--max-gap 120] [--min-faces 3] [--min-pixels 20000]
                                         [--labels IN --merged OUT] <clothes.npy> <output.json>

`track` and `extract` take the reference's arguments and options and write byte-compatible files (track.txt, landmarks.txt,
embedding.txt: formats.py).  `cluster` is the verb BASELINE.json's north_star names; the reference offers clustering through the API
only (face/clustering.py:130-134).  It writes `identifier label` lines, the file `demo --label` reads (pyannote-face.py:87,391-397).
`enroll` / `enroll-track` / `identify` (identification.py; no reference verb) name tracks or clusters against a gallery of enrolled faces:
`identify` writes `identifier name` lines, the same file `demo --label` reads; `process --gallery` does it in the same run.
`search` (search.py; no reference verb; SEARCH.md) answers "where else does this face appear?": the exact k nearest faces of one or more
embedding files to a track or to a person of a gallery, one `rank distance path track T` line per hit, nearest first.
`cast` (cast.py; no reference verb; CAST.md) answers "who are the people of these films?": rank-order clustering on the exact k-NN graph of
the tracks (or faces) of any number of embedding files, one `path track person` line per (file, track).
`demo` (pyannote-face.py:317-413) writes the video with the tracks, their numbers and labels and, with --landmark, the nose lines drawn
on it, as a YUV4MPEG2 stream: to a `.y4m` path, or to stdout for `-` (`... demo film.y4m track.txt - | ffmpeg -i - out.mp4`).  Resize,
drawing and RGB -> YUV 4:2:0 run in one kernel on the GPU (DEMO.md states every pixel; the font is the project's own, not OpenCV's
Hershey).  Audio is not carried: the reference hands the source's audio track to moviepy, a Y4M stream has none.
`redact` (no reference verb; REDACT.md) writes the same stream with the faces of the chosen tracks pixelated, blended or filled: a cell-mean
reduction on the GPU in front of the same kernel.  It hides what the tracking file holds; a face the detector never found stays visible.

`faces` (no reference verb; FACES.md) writes a contact sheet -- for every track, or with --label every cluster or name, its few best
faces side by side -- as a binary PPM (a `.ppm` path, or `-` for stdout) or a `.npy` array: who is cluster 7?  Best is computed on the
GPU, a sharpness and exposure reduction over every face chip of the film; the sheet is composed there too.
`talk` (no reference verb; TALK.md) writes one line per face with how much its mouth moved since the frame before -- displaced absolute
differences of the aligned chip's mouth window, less those of a control window above it, computed on the GPU -- and, with --segments,
the spans in which a track is taken to be talking: a stated rule with untuned thresholds on top of the per-face columns.

`storyboard` (no reference verb; STORYBOARD.md) writes the shots of `shot` as a contact sheet -- a few frames of every shot, whole, as
thumbnails under the shot's number and start, coloured and with --by thread lined up by the threads of `thread` -- as a binary PPM or a
`.npy` array: what is shot 212, and is thread C one camera set-up?  The thumbnails are exact area averages made on the GPU.
`scene` (pyannote-structure.py scene, which the reference leaves unimplemented) writes the scenes of a thread file.
`fingerprint` (no reference verb; REPEAT.md) writes a 128-bit print of every frame, made on the GPU from the frame's 9 x 9 thumbnail, as a
uint64 [n][4] `.npy`; `repeat` compares print files with themselves and with each other and writes the stretches they share -- a recap,
the titles, a rerun -- as JSON.  The thresholds are untuned; the runs and segments are the product.
`blend` (no reference verb; BLEND.md) writes the blend record of every frame -- how far the luma of a small thumbnail lies from the frames
4, 8, 16 and 32 before it, and how far the frame in the middle lies off the line between the two, summed on the GPU -- as a uint32 [n][16]
`.npy`; `transition` reads that file alone and writes the fades, dissolves and blank stretches it shows as JSON and, with --shots and
--refined, the shots of `shot` cut at them, which `track`, `thread` and `storyboard` read unchanged.  The thresholds are untuned.
`motion` (no reference verb; MOTION.md) fits a similarity -- translation, zoom, roll -- to the dense flow the shot detector computes between
every two consecutive frames, on the GPU and in integers, and writes 80 bytes a frame as an int64 [n][10] `.npy`; `camera` reads that file
alone and writes the pans, tilts, zooms and static stretches it shows as JSON.  `transition --motion` marks the spans that lie inside a
camera move as `camera` instead of a dissolve.  The thresholds are untuned.
`text` (no reference verb; CAPTION.md) measures overlaid text -- name straps, subtitles, title cards -- on every pixel of every frame at
full resolution, on the GPU and in integers: per 16 x 16 cell the pixels with a strong horizontal luma difference that were there, unmoved,
in the frame before, and one mask bit a cell, as a uint32 [n][8 + ch wpr] `.npy`; `caption` reads that file alone and writes the
captions it shows -- when, and in which box of the picture -- as JSON, with --tracking also the tracks on screen with each.  No
characters are read.  The thresholds are untuned.
`clothes` (no reference verb; CLOTHES.md) measures what a person wears: a colour histogram of 256 bins, summed on the GPU and in integers over
the torso windows under the faces of every track, as an int64 [T][6 + 256 bands] `.npy`; `link` reads that file alone and writes which
tracks wear the same clothes -- mutual best matches by histogram intersection, with a margin -- as JSON and, with --labels and --merged,
the label file of `cluster` or `identify` merged along those links.  No body is detected.  The thresholds are untuned.

<video>: no codec is linked (reference video.py:345-406 runs ffmpeg); the verbs read what a decoder writes --
  * a YUV4MPEG2 file (`.y4m`, or any file that starts with `YUV4MPEG2`): 8-bit 4:2:0 / 4:2:2 / 4:4:4, memory mapped, frame rate from
    its header (`ffmpeg -i film.mkv -pix_fmt yuv420p -f yuv4mpegpipe film.y4m`); the planes go to the GPU as they are and are
    converted to RGB there (--matrix 601|709, --range limited|full override the header);
  * `-`: the same stream from stdin, for the verbs that read the video once and need no length (`track`, `process`, `talk`, `fingerprint`, `blend`, `motion`, `text`, `clothes`):
    `ffmpeg -i film.mkv -pix_fmt yuv420p -f yuv4mpegpipe - | python -m pyannote_video_amd process - ...`;
  * a `.npy` file holding uint8 [N, H, W, 3] RGB frames (memory mapped; frame rate from --fps);
  * the bench's synthetic clip: `synthetic:<width>x<height>x<frames>[:shots[:faces[:seed]]]`.
<shot.json>: a JSON list of [start, end] seconds (what pyannote.core.json holds for a Timeline reduces to this for our purpose).
"""
import argparse
import json
import sys
import numpy as np
from . import formats

MIN_OVERLAP_RATIO = 0.5      # pyannote-face.py:112-114
MIN_CONFIDENCE = 10.
MAX_GAP = 1.


class NpyVideo(object):
    """decoded frames with the iteration contract of the reference's Video (video.py:411-464): yields (t, uint8 HxWx3 RGB)"""

    def __init__(self, path, frame_rate=25.0):
        self._frames = np.load(path, mmap_mode="r")
        if self._frames.dtype != np.uint8 or self._frames.ndim != 4 or self._frames.shape[3] != 3:
            raise IOError("%s: expected uint8 frames of shape [N, H, W, 3]" % path)
        self.frame_rate = float(frame_rate)
        self._size = (int(self._frames.shape[2]), int(self._frames.shape[1]))
        self._frame_size = self._size
        self.duration = len(self._frames) / self.frame_rate
        self.step, self.start, self.end = 1.0 / self.frame_rate, 0.0, self.duration      # what structure.Shot reads (video.py:186-190)

    @property
    def size(self):
        return self._size

    @property
    def frame_size(self):
        return self._frame_size

    @frame_size.setter
    def frame_size(self, value):
        self._frame_size = tuple(int(v) for v in value)     # applied by the consumer on the device (FaceTracking: detect_min_size)

    def __len__(self):
        return len(self._frames)

    def __iter__(self):
        for i in range(len(self._frames)):
            yield i / self.frame_rate, np.ascontiguousarray(self._frames[i])

    def frame(self, i):
        return np.ascontiguousarray(self._frames[i])

    def __call__(self, t):
        """the frame at time t: index int(fps * t + 1e-5), as the reference's Video reads it (video.py:466-486)"""
        i = int(self.frame_rate * t + 0.00001)
        if not 0 <= i < len(self._frames):
            raise IOError("no frame at t = %.3f" % t)
        return self.frame(i)


def open_video(spec, frame_rate, matrix=None, full_range=None):
    """matrix ('601' / '709') and full_range (bool) override what a Y4M header says; None leaves it to the header"""
    if spec == "-":
        from .y4m import Y4mVideo
        return Y4mVideo(sys.stdin.buffer, frame_rate, matrix=matrix, full_range=full_range)
    if spec.startswith("synthetic:"):
        from . import synth
        parts = spec[len("synthetic:"):].split(":")
        w, h, n = (int(v) for v in parts[0].lower().split("x"))
        kw = {}
        for name, val in zip(("n_shots", "faces", "seed"), parts[1:]):
            kw[name] = int(val)
        return synth.SyntheticVideo(width=w, height=h, n_frames=n, frame_rate=frame_rate, **kw)
    from . import y4m
    if y4m.is_y4m(spec):
        return y4m.Y4mVideo(spec, frame_rate, matrix=matrix, full_range=full_range)
    return NpyVideo(spec, frame_rate)


class _Shot(object):
    def __init__(self, start, end):
        self.start, self.end = float(start), float(end)


def load_shots(path):
    with open(path) as f:
        data = json.load(f)
    if isinstance(data, dict):                      # pyannote.core.json Timeline: {"pyannote": "Timeline", "content": [{"start":..,"end":..}]}
        data = [(s["start"], s["end"]) for s in data.get("content", [])]
    return [_Shot(a, b) for a, b in data]


def auto_detect_batch(width, height):
    """frames whose pyramids and feature maps are resident together: 128 at 1080p (18 GB), fewer for larger frames"""
    return int(max(8, min(128, 128 * (1920 * 1080) // max(int(width) * int(height), 1))))


def _pipeline(video, ctx, landmark_model=None, embedding_model=None, **kw):
    from . import pipeline, runtime
    ctx = ctx or runtime.default_context()
    w, h = video.size
    return pipeline.FacePipeline(ctx, landmark_model, embedding_model, detect_batch_size=auto_detect_batch(w, h), **kw)


def track(video, shot, output, detect_min_size=0.0, detect_every=0.0, track_min_overlap_ratio=MIN_OVERLAP_RATIO,
          track_min_confidence=MIN_CONFIDENCE, track_max_gap=MAX_GAP, ctx=None):
    """Tracking by detection (pyannote-face.py:239-269): track.txt, one line per (track, frame), flushed per track.  The video is read
    once, in a thread of its own, into the pinned ingest ring; shots go through the streaming engine (engine.py): batched detection,
    bulk tracker work, the state machine one shot behind, frames released shot by shot."""
    pipe = _pipeline(video, ctx, detect_min_size=detect_min_size, detect_every=detect_every, track_min_overlap_ratio=track_min_overlap_ratio,
                     track_min_confidence=track_min_confidence, track_max_gap=track_max_gap)
    shots = _load(shot, load_shots)
    with open(output, 'w') as foutput:
        tm = {}
        res = pipe.run_stream(video, shots, extract=False, cluster=False, on_tracks=_track_writer(foutput), timings=tm)
        res["timings"] = tm
        return res


def _track_writer(foutput):
    """the on_tracks of `track` and `process`: the finished tracks, numbered from 0 as they come, one line per (track, frame), flushed
    per track"""
    import itertools
    numbers = itertools.count()

    def write(tracks):
        for trk in tracks:
            for line in formats.track_lines(next(numbers), trk):
                foutput.write(line)
            foutput.flush()
    return write


def _jitter_kw(num_jitters, jitter_seed):
    """what landmarks_embed gets beyond the faces: nothing without jitters (the call of before), else num_jitters and the seed"""
    if int(num_jitters) < 0:
        raise ValueError("--jitters must not be negative")
    return {"num_jitters": int(num_jitters), "seed": int(jitter_seed)} if num_jitters else {}


def extract(video, landmark_model, embedding_model, tracking, landmark_output, embedding_output, ctx=None, batch=2048, ahead=96,
            num_jitters=0, jitter_seed=0):
    """Facial features (pyannote-face.py:271-314): landmarks.txt and embedding.txt for every face of the track file.  The faces
    are paired with frames by getFaceGenerator's rules (pipeline.faces_per_frame); a reader thread pushes the frames that carry faces
    through the pinned ingest ring (asynchronous uploads, at most `ahead` frames in flight) while this thread computes `batch` faces per
    library call and writes the lines in the reference's order.  num_jitters > 1: every descriptor is the mean over that many jittered
    chips (dlib's compute_face_descriptor(img, shape, num_jitters); JITTER.md)."""
    import queue
    import threading
    from . import pipeline, runtime
    from .feed import FrameFeed
    jitter = _jitter_kw(num_jitters, jitter_seed)
    ctx = ctx or runtime.default_context()
    ctx.load_shape_predictor(landmark_model)
    ctx.load_embedder(embedding_model)
    frame_width, frame_height = video.frame_size
    rows = formats.read_tracks(tracking)
    want = {}
    for fi, T, g in pipeline.faces_per_frame(rows, _frame_times(video, rows), frame_width, frame_height):
        want[fi] = (T, g)
    state = {"error": None}                  # the writer thread's
    with FrameFeed(ctx, video, want, ahead=ahead, name="pvface-extract-reader") as feed, \
            open(landmark_output, 'wb') as flandmark, open(embedding_output, 'wb') as fembedding:
        wq = queue.Queue(maxsize=4)

        def writer():
            # the text of batch i is formatted (in the library, outside the GIL) and written while the GPU computes batch i + 1
            try:
                while True:
                    item = wq.get()
                    if item is None:
                        return
                    if state["error"] is not None:
                        continue
                    T, ident, pts, emb = item
                    flandmark.write(formats.landmark_rows(T, ident, pts, frame_width, frame_height))
                    fembedding.write(formats.embedding_rows(T, ident, emb))
            except BaseException as e:          # noqa: BLE001 -- re-raised below
                state["error"] = e
                while wq.get() is not None:
                    pass

        wth = threading.Thread(target=writer, name="pvface-extract-writer")
        wth.start()
        try:
            for part in feed.batches(batch, lambda fi: len(want[fi][1])):
                if state["error"] is not None:
                    break
                jobs = [(dev, box, want[fi][0], ident) for fi, dev in part for ident, box in want[fi][1]]
                pts, emb = ctx.landmarks_embed([j[0] for j in jobs], [j[1] for j in jobs], **jitter)
                wq.put(([j[2] for j in jobs], [j[3] for j in jobs], pts, emb))
                feed.release_all(dev for _, dev in part)
        finally:
            wq.put(None)
            wth.join()
    if state["error"] is not None:
        raise state["error"]


def process(video, shot, landmark_model, embedding_model, tracking_output, landmark_output, embedding_output, label_output=None,
            detect_min_size=0.0, detect_every=0.0, track_min_overlap_ratio=MIN_OVERLAP_RATIO, track_min_confidence=MIN_CONFIDENCE,
            track_max_gap=MAX_GAP, threshold=0.6, ctx=None, do_not_cooccur=False, gallery=None, identify_threshold=0.6, unknown=None):
    """`track` + `extract` (+ `cluster`) in ONE pass over the video -- one decode, one upload per frame; the reference needs two decodes
    (pyannote-face.py:261 and :287).  Writes the same three files as the separate verbs, line for line (the faces of one frame in the
    order pandas' sort of the complete track table gives them: formats.file_order), plus the `identifier label` file of `cluster`.
    gallery (needs label_output): the clusters are identified from the rows the run itself produced, the labels file carries names for
    the matched clusters and cluster numbers for the rest -- exactly what `identify --labels` writes from the files of the same run."""
    if gallery is not None and label_output is None:
        raise ValueError("process: --gallery names clusters, it needs --labels")
    pipe = _pipeline(video, ctx, landmark_model, embedding_model, detect_min_size=detect_min_size, detect_every=detect_every,
                     track_min_overlap_ratio=track_min_overlap_ratio, track_min_confidence=track_min_confidence, track_max_gap=track_max_gap,
                     threshold=threshold, constraint="cooccur" if do_not_cooccur else None)
    shots = _load(shot, load_shots)
    with open(tracking_output, 'w') as foutput:
        tm = {}
        res = pipe.run_stream(video, shots, on_tracks=_track_writer(foutput), cluster=label_output is not None, timings=tm)
        res["timings"] = tm
    w, h = video.size
    with open(landmark_output, 'wb') as flandmark, open(embedding_output, 'wb') as fembedding:
        flandmark.write(formats.landmark_rows(res["face_T"], res["face_id"], res["landmarks"], w, h))
        fembedding.write(formats.embedding_rows(res["face_T"], res["face_id"], res["embeddings"]))
    if label_output is not None and gallery is None:
        with open(label_output, 'w') as f:
            for identifier in sorted(set(res["face_id"].tolist())):
                f.write('{identifier:d} {label:d}\n'.format(identifier=identifier, label=res["labels"].get(identifier, identifier)))
    elif label_output is not None:
        from . import identification, _lib
        tracks = sorted(set(res["face_id"].tolist()))
        label = {t: int(res["labels"].get(t, t)) for t in tracks}
        res["identification"] = []
        if tracks:
            # the rows as `identify` reads them back from the files written above: 3-decimal times, 5-decimal values, file order
            T = np.array([formats.quantise_time(t) for t in res["face_T"]], np.float64)
            X = res["X"] if res.get("X") is not None else _lib.round_rows(res["embeddings"], 5)
            ident = identification.FaceIdentification(gallery, threshold=identify_threshold, ctx=pipe.ctx)
            res["identification"] = ident.scores_arrays(res["face_id"], X, label, T)
        identification.write_identification(label_output, res["identification"], tracks, label, unknown, per_cluster=True)
    return res


def _load(value, reader):
    """what a verb was given for one of its input files: a path, read here, or the content as `reader` returns it"""
    return reader(value) if isinstance(value, str) else value


def _frame_times(video, rows):
    """the time of every frame; of a stream, which has no length, of as many frames as the tracking rows need"""
    try:
        n_frames = len(video)
    except TypeError:
        n_frames = int(max([r[0] for r in rows] or [0.0]) * video.frame_rate) + 2
    return [i / video.frame_rate for i in range(n_frames)]


def _save_array(output, array):
    """a verb's table as a .npy file: `output` is a path, or an open binary file"""
    if hasattr(output, "write"):
        np.save(output, array)
    else:
        with open(output, "wb") as fo:
            np.save(fo, array)


def _write_json(output, doc):
    """a verb's findings as JSON: `output` is a path, or - for stdout"""
    text = json.dumps(doc, indent=1) + "\n"
    if str(output) == "-":
        sys.stdout.write(text)
        sys.stdout.flush()
    else:
        with open(output, "w") as fo:
            fo.write(text)


def _check_sheet_name(verb, output):
    if not (str(output) == "-" or str(output).endswith((".ppm", ".npy"))):
        raise ValueError("%s: the output is a .ppm or .npy path, or - for a PPM on stdout" % verb)


def _write_sheet(output, sheet):
    """a contact sheet, uint8 [H, W, 3]: a binary PPM to a `.ppm` path or, for -, to stdout; the array itself to a `.npy` path"""
    from .faces import ppm_bytes
    if str(output).endswith(".npy"):
        np.save(output, sheet)
    elif str(output) == "-":
        sys.stdout.buffer.write(ppm_bytes(sheet))
        sys.stdout.buffer.flush()
    else:
        with open(output, "wb") as fo:
            fo.write(ppm_bytes(sheet))


def cluster(embeddings, output, threshold=0.6, force=False, metric="euclidean", ctx=None, do_not_cooccur=False):
    """FaceClustering on an embedding file (face/clustering.py:130-134) -> `identifier label` lines for `demo --label`.
    Tracks that take no part in the clustering (a single timestamp: clustering.py:78-79) keep their own identifier as label.
    do_not_cooccur: tracks whose extents intersect never get the same label (clustering.py:142-143, FaceClustering(constraint='cooccur'))."""
    from .clustering import FaceClustering
    clustering = FaceClustering(threshold=threshold, force=force, metric=metric, ctx=ctx, constraint="cooccur" if do_not_cooccur else None)
    starting_point, features = clustering.model.preprocess(embeddings)
    result = clustering(starting_point, features=features)
    label = {int(track): int(lab) for _, track, lab in result.itertracks(yield_label=True)}
    with open(output, 'w') as f:
        for identifier in sorted(set(int(t) for t in np.unique(features.track))):
            f.write('{identifier:d} {label:d}\n'.format(identifier=identifier, label=label.get(identifier, identifier)))
    return label


def identify(embeddings, gallery, output, threshold=0.6, metric="euclidean", labels=None, unknown=None, scores=None, ctx=None):
    """Names for the tracks of an embedding file -> `identifier name` lines for `demo --label`.  Without `labels` the decision is made
    per track: a track nobody matches is left out (or gets `unknown`).  With `labels` (a `cluster` output) it is made per cluster: every
    track of a matched cluster gets the name, a track of an unmatched one keeps its cluster label (or gets `unknown`), and the file
    replaces the `cluster` file.  scores: one line per group, `group best_name best_dist second_name second_dist` -- the nearest
    identity even above the threshold, `-` for a missing name."""
    from . import identification
    ident = identification.FaceIdentification(gallery, threshold=threshold, metric=metric, ctx=ctx)
    time, track, X = formats.read_embeddings(embeddings)
    label = identification.read_label_map(labels) if labels is not None else {}
    result = ident.scores_arrays(track, X, label or None, time)
    identification.write_identification(output, result, np.unique(track).tolist(), label, unknown, per_cluster=labels is not None,
                                        scores_output=scores)
    return {g: (name if matched else None, bd, second, sd) for g, name, bd, second, sd, matched in result}


def search(output, embeddings, k=100, max_distance=None, rows=False, include_self=False, gallery=None, name=None, source=None, track=None,
           ctx=None):
    """The k nearest faces of the embedding files to a query -- the rows of a person of a gallery (`gallery`, `name`) or of a track of an
    embedding file (`source`, `track`) -- as `rank distance path track T` lines, nearest first (`output`: a path, or - for stdout).
    Without `rows` only the best hit of each (file, track) among the k is kept: the tracks that own the k nearest faces.  A query taken
    from a track of a searched file does not find its own track, unless `include_self`.  -> the hits"""
    from . import search as _search
    if (gallery is None) == (source is None) or (gallery is not None and name is None) or (source is not None and track is None):
        raise ValueError("search: the query is --gallery PATH --name NAME, or --from EMBEDDINGS --track ID")
    if not 1 <= int(k) <= _search.MAX_K:
        raise ValueError("search: k must lie in 1 .. %d" % _search.MAX_K)
    fs = _search.FaceSearch(ctx=ctx)
    for path in embeddings:
        fs.add(path)
    if len(fs) == 0:
        raise ValueError("search: the table is empty (no row in %s)" % ", ".join(embeddings))
    own = -1
    if gallery is not None:
        query = fs.rows_of_person(gallery, name)
    else:
        query = fs.rows_of_track(source, track)
        own = -1 if include_self else fs.group_of(source, track)
    hits = fs.search(query, k=k, max_distance=max_distance, exclude_group=own, collapse=not rows)
    _search.write_hits(output, hits)
    return hits


def cast(output, embeddings, k=64, max_distance=0.6, threshold=2.0, by="track", labels=None, graph=None, ctx=None):
    """The persons of one or more embedding files: `path track person` lines, one per (file, track), in the order of the files and then
    by track (`output`: a path, or - for stdout); persons are numbered 0, 1, ... .  labels: a suffix -- `<embeddings><suffix>` gets the
    file's `identifier label` lines for `demo --label`; graph: a path that gets the k-NN lists as an .npz.  -> the lines"""
    from . import cast as _cast
    fc = _cast.FaceCast(ctx=ctx)
    for path in embeddings:
        fc.add(path)
    lines = fc.run(k=k, max_distance=max_distance, threshold=threshold, by=by, graph=graph)
    _cast.write_cast(output, lines)
    if labels is not None:
        _cast.write_label_files(lines, labels)
    return lines


def enroll_track(embeddings, track, name, gallery, append=False):
    """the rows of one track of an embedding file, under a name: how a person who appears in the video gets enrolled"""
    from . import identification
    formats.check_gallery_name(name)
    _, ids, X = formats.read_embeddings(embeddings)
    rows = X[ids == int(track)]
    if len(rows) == 0:
        raise ValueError("%s has no row of track %d" % (embeddings, int(track)))
    identification.FaceGallery().add(name, rows).save(gallery, append=append)
    return len(rows)


def enroll(video, landmark_model, embedding_model, name, gallery, append=False, ctx=None, batch=16, num_jitters=0, jitter_seed=0):
    """Every frame of the video through detector -> landmarks -> embedder; the detection of largest area is enrolled (the first in
    detector order on equal areas), frames without a face are skipped.  num_jitters > 1: every enrolled descriptor is the mean over that
    many jittered chips (JITTER.md).  -> {"faces": enrolled, "skipped": frames without a face}"""
    import os
    from . import identification, runtime
    formats.check_gallery_name(name)
    jitter = _jitter_kw(num_jitters, jitter_seed)
    if not append and os.path.exists(gallery):
        raise FileExistsError("%s exists: --append adds to it" % gallery)          # before any work
    ctx = ctx or runtime.default_context()
    ctx.load_shape_predictor(landmark_model)
    ctx.load_embedder(embedding_model)
    rows, skipped, pending = [], 0, []

    def flush():
        frames = [ctx.upload(rgb) for rgb in pending]
        try:
            keep_f, keep_b = [], []
            for f, (boxes, _) in zip(frames, ctx.detect_batch(frames, 1)):
                if boxes:
                    area = [(b[2] - b[0] + 1) * (b[3] - b[1] + 1) for b in boxes]
                    keep_f.append(f); keep_b.append(boxes[area.index(max(area))])
            if keep_b:
                rows.append(ctx.landmarks_embed(keep_f, keep_b, **jitter)[1])
            return len(frames) - len(keep_b)
        finally:
            for f in frames:
                f.release()
            del pending[:]
    for _, rgb in video:
        pending.append(rgb)
        if len(pending) >= batch:
            skipped += flush()
    if pending:
        skipped += flush()
    if not rows:
        raise ValueError("enroll: no face was found in the video")
    E = np.concatenate(rows)
    identification.FaceGallery().add(name, E).save(gallery, append=append)
    return {"faces": int(len(E)), "skipped": int(skipped)}


def shot(video, output, height=50, window=2.0, threshold=1.0, ctx=None):
    """Shot boundary detection (scripts/pyannote-structure.py:65-70): a pyannote.core.json Timeline file that `track` reads back"""
    from .structure import Shot
    segments = sorted(Shot(video, height=height, context=window, threshold=threshold, ctx=ctx))
    with open(output, 'w') as fp:
        json.dump({"pyannote": "Timeline", "content": [{"start": s.start, "end": s.end} for s in segments]}, fp)
    return segments


def thread(video, shot, output, min_match=20, lookahead=24, ctx=None):
    """Shot threading (scripts/pyannote-structure.py:72-80): reads what `shot` writes, writes a pyannote.core.json Annotation"""
    from .structure import Thread, Segment
    shots = [Segment(s.start, s.end) for s in _load(shot, load_shots)]
    threads = Thread(video, shot=shots, lookahead=lookahead, min_match=min_match, ctx=ctx)()
    with open(output, 'w') as fp:
        json.dump(threads.for_json(), fp)
    return threads


def scene(video, thread, output):
    """Scenes (scripts/pyannote-structure.py:39 usage; its body raises NotImplementedError): the threads of `thread` with every
    biconnected component of three or more shots relabelled (structure.thread_scenes).  The video is not opened: scenes are a function
    of the threads alone."""
    from .structure import thread_scenes
    from ._core import Annotation
    with open(thread) as fp:
        threads = Annotation.from_json(json.load(fp))
    scenes = thread_scenes(threads)
    with open(output, 'w') as fp:
        json.dump(scenes.for_json(), fp)
    return scenes


def storyboard(video, shot, output, per=1, width=160, columns=None, thread=None, by="time", t_from=0.0, t_until=None, index=None,
               batch=64, ctx=None):
    """The shots of a film as a contact sheet (STORYBOARD.md): `per` frames of every shot, whole, as thumbnails `width` pixels wide under
    a caption, coloured by thread with `thread` (what `thread` or `scene` wrote).  The frames are read by one seeking FrameFeed and
    reduced on the device `batch` at a time (storyboard.build).  Returns {"width", "height", "shots", "tiles"}."""
    from . import storyboard as _board, runtime
    from ._core import Annotation
    _check_sheet_name("storyboard", output)
    shots = list(_load(shot, load_shots))
    annotation = None
    if thread is not None:
        if isinstance(thread, str):
            with open(thread) as fp:
                annotation = Annotation.from_json(json.load(fp))
        else:
            annotation = thread
    ctx = ctx or runtime.default_context()
    sheet, lines, res = _board.build(ctx, video, shots, _board.shot_labels(shots, annotation), per=per, width=width, columns=columns, by=by,
                                     t_from=t_from, t_until=t_until, batch=batch)
    if index:
        with open(index, "w") as fx:
            fx.write("".join(lines))
    _write_sheet(output, sheet)
    return res


def fingerprint(video, output, t_from=0.0, t_until=None, batch=64, ctx=None, ahead=96):
    """A print of every frame of the video whose time lies in [t_from, t_until) (REPEAT.md): one streaming pass, a reader thread pushes
    the frames through the pinned ingest ring (RGB or YUV), this thread asks for the prints of `batch` resident frames per library call
    (32 bytes a frame come back) and releases them.  Writes uint64 [n][4] -- H, V, SY | RANGE << 32, ms(T) | frame index << 32 -- as
    a .npy file (`output` may be an open binary file).  Returns {"frames", "first"}."""
    from . import repeat as _repeat, runtime
    from .feed import FrameFeed, frame_range
    if int(batch) < 1:
        raise ValueError("fingerprint: a batch holds at least one frame")
    first, end = frame_range(video, t_from, t_until)
    ctx = ctx or runtime.default_context()
    parts = []
    with FrameFeed(ctx, video, _repeat.EveryFrame(first, end), ahead=max(ahead, 2 * int(batch)), name="pvface-fingerprint-reader") as feed:
        for part in feed.batches(batch):
            frames = [dev for _, dev in part]
            parts.append(ctx.frame_prints(frames))
            feed.release_all(frames)
    prints = _repeat.stamp(np.concatenate(parts) if parts else np.zeros((0, 4), np.uint64), first, video.frame_rate)
    _save_array(output, prints)
    return {"frames": int(len(prints)), "first": first}


def repeat(output, prints, max_bits=10, flat=16, min_duration=2.0, max_gap=0.5, min_separation=5.0, ctx=None):
    """The stretches print files share with themselves and with each other (REPEAT.md): every file against itself, beyond
    `min_separation` seconds, and against every later one; the runs of matching prints come from the device (Context.print_runs), the
    rest is repeat.py.  Writes a JSON list of {a, b, a_start, a_end, b_start, b_end, frames, offset} and returns it."""
    from . import repeat as _repeat, runtime
    if not prints:
        raise ValueError("repeat: no print files")
    if not 0 <= int(max_bits) <= 128:
        raise ValueError("repeat: --max-bits is 0 .. 128")
    files = [(str(p), _repeat.load(p)) for p in prints]
    found = _repeat.compare(ctx or runtime.default_context(), files, max_bits=max_bits, flat=flat, min_duration=min_duration, max_gap=max_gap,
                            min_separation=min_separation)
    _write_json(output, found)
    return found


def blend(video, output, width=64, t_from=0.0, t_until=None, batch=64, ctx=None, ahead=96):
    """The blend record of every frame of the video whose time lies in [t_from, t_until) (BLEND.md): one streaming pass as `fingerprint`
    makes it; `batch` resident frames per frame_blend call, the last 32 luma planes carried into the next call (blend.Carry), so the
    file does not depend on `batch`.  The thumbnail is `width` pixels wide and keeps the frame's aspect.  Writes uint32 [n][16], stamped
    with ms(T) and the frame index, as a .npy file (`output` may be an open binary file).  Returns {"frames", "first", "tw", "th"}."""
    from . import blend as _blend, repeat as _repeat, runtime
    from .feed import FrameFeed, frame_range
    if int(batch) < 1:
        raise ValueError("blend: a batch holds at least one frame")
    if int(width) < 1:
        raise ValueError("blend: --width is at least 1")
    w, h = video.frame_size
    tw, th = _blend.tile_size(width, w, h)
    first, end = frame_range(video, t_from, t_until)
    ctx = ctx or runtime.default_context()
    carry = _blend.Carry(ctx, tw, th)
    parts = []
    with FrameFeed(ctx, video, _repeat.EveryFrame(first, end), ahead=max(ahead, 2 * int(batch)), name="pvface-blend-reader") as feed:
        for part in feed.batches(batch):
            rows, done = carry.measure([dev for _, dev in part])
            parts.append(rows)
            feed.release_all(done)
    rows = _blend.stamp(np.concatenate(parts) if parts else np.zeros((0, _blend.WORDS), np.uint32), first, video.frame_rate)
    _save_array(output, rows)
    return {"frames": int(len(rows)), "first": first, "tw": tw, "th": th}


def transition(rows, output, move=4.0, linear=0.25, flat=2.0, min_duration=0.12, shots=None, refined=None, motion=None):
    """Fades, dissolves and blank stretches from a blend file (BLEND.md), on the host: a JSON list of {kind, start, end, first, last}.
    With `shots` (what `shot` wrote) and `refined`, also the Timeline of `shot` cut at the middle of every dissolve and of every blank
    run a fade ends in or starts from.  With `motion` (what `motion` wrote for the same video), a span with more than half of its frames
    inside a pan, tilt or zoom of `camera`'s default rules is written as `camera` and cuts nothing.  The video is not opened.  Returns
    the list."""
    from . import blend as _blend
    if (shots is None) != (refined is None):
        raise ValueError("transition: --shots and --refined go together")
    table = _blend.load(rows) if isinstance(rows, str) else np.ascontiguousarray(rows)
    more = {}
    if motion is not None:
        from . import motion as _motion
        more["moving"] = _motion.moving_frames(_motion.load(motion, "transition") if isinstance(motion, str) else np.ascontiguousarray(motion))
    found, cuts = _blend.analyse(table, move=move, linear=linear, flat=flat, min_duration=min_duration, **more)
    listed = _blend.report(table, found)
    _write_json(output, listed)
    if shots is not None:
        before = [(s.start, s.end) for s in _load(shots, load_shots)]
        pieces = _blend.refine(before, [int(table[c, 12]) / 1000.0 for c in cuts])
        with open(refined, "w") as fp:
            json.dump({"pyannote": "Timeline", "content": [{"start": a, "end": b} for a, b in pieces]}, fp)
    return listed


def motion(video, output, width=96, t_from=0.0, t_until=None, batch=256, ctx=None, ahead=96):
    """The motion row of every frame of the video whose time lies in [t_from, t_until) (MOTION.md): one streaming pass as `blend` makes
    it.  The small image is `width` pixels wide and keeps the frame's aspect: the shot detector's gray, bilinear image, of which the
    library computes the dense flow between every two consecutive frames and fits the camera's motion to it.  `batch` resident frames
    per shot_motion call; a batch's last frame stays resident as the first frame of the next call (motion.Pairs), so the file does not
    depend on `batch`.  The first frame of the range has no frame before it and gets a row without valid pixels.  Writes int64 [n][10],
    stamped with ms(T) | index << 32, as a .npy file (`output` may be an open binary file).  Returns {"frames", "first", "tw", "th"}."""
    from . import motion as _motion, repeat as _repeat, runtime
    from .feed import FrameFeed, frame_range
    if int(batch) < 1:
        raise ValueError("motion: a batch holds at least one frame")
    if int(width) < 1:
        raise ValueError("motion: --width is at least 1")
    w, h = video.frame_size
    tw, th = _motion.tile_size(width, w, h)
    first, end = frame_range(video, t_from, t_until)
    ctx = ctx or runtime.default_context()
    carry = _motion.Pairs(ctx, tw, th)
    parts = []
    with FrameFeed(ctx, video, _repeat.EveryFrame(first, end), ahead=max(ahead, 2 * int(batch)), name="pvface-motion-reader") as feed:
        for part in feed.batches(batch):
            rows, done = carry.measure([dev for _, dev in part])
            parts.append(rows)
            feed.release_all(done)
    rows = _motion.stamp(np.concatenate(parts) if parts else np.zeros((0, _motion.WORDS), np.int64), first, video.frame_rate)
    _save_array(output, rows)
    return {"frames": int(len(rows)), "first": first, "tw": tw, "th": th}


def camera(rows, output, pan=5.0, zoom=3.0, window=0.5, min_inliers=50, min_duration=0.5, max_gap=0.2, shots=None):
    """Pans, tilts, zooms and static stretches from a motion file (MOTION.md), on the host: a JSON list of {kind, start, end, first, last,
    rate}.  With `shots` (what `shot` wrote) no pair that straddles a shot boundary counts and no span crosses one.  The video is not
    opened.  Returns the list."""
    from . import motion as _motion
    table = _motion.load(rows) if isinstance(rows, str) else np.ascontiguousarray(rows)
    if shots is not None:
        shots = [(s.start, s.end) for s in _load(shots, load_shots)]
    found = _motion.analyse(table, pan=pan, zoom=zoom, window=window, min_inliers=min_inliers, min_duration=min_duration, max_gap=max_gap,
                            shots=shots)
    listed = _motion.report(table, found)
    _write_json(output, listed)
    return listed


def text(video, output, step=0.0, edge=48, still=8, on=24, t_from=0.0, t_until=None, batch=64, ctx=None, ahead=96):
    """The text record of the frames of the video whose time lies in [t_from, t_until) (CAPTION.md): one streaming pass as `blend` makes
    it, at full resolution.  Every k-th frame from the first is measured, k = max(1, floor(step * rate + 1 / 2)), against the measured
    frame before it.  `batch` resident frames per frame_text call; a batch's last frame stays resident as `prev` of the next call
    (text.Carry), so the file does not depend on `batch`.  Writes uint32 [n][8 + ch wpr], stamped with ms(T) and the frame index, as a
    .npy file (`output` may be an open binary file).  Returns {"frames", "first", "every"}."""
    from . import text as _text, runtime
    from .feed import EveryKth, FrameFeed, frame_range
    if not 1 <= int(batch) <= _text.MAX_FRAMES:
        raise ValueError("text: a batch holds 1 .. %d frames" % _text.MAX_FRAMES)
    if step < 0:
        raise ValueError("text: --step is not negative")
    w, h = video.frame_size
    if not (1 <= w <= _text.MAX_SIDE and 1 <= h <= _text.MAX_SIDE):
        raise ValueError("text: frames of %d x %d; sides of at most %d are measured" % (w, h, _text.MAX_SIDE))
    k = _text.every(step, video.frame_rate)
    first, end = frame_range(video, t_from, t_until)
    ctx = ctx or runtime.default_context()
    carry = _text.Carry(ctx, edge=edge, still=still, on=on)
    parts = []
    with FrameFeed(ctx, video, EveryKth(first, end, k), ahead=max(ahead, 2 * int(batch)), name="pvface-text-reader") as feed:
        for part in feed.batches(batch):
            rows, done = carry.measure([dev for _, dev in part])
            parts.append(rows)
            feed.release_all(done)
    rows = _text.stamp(np.concatenate(parts) if parts else np.zeros((0, _text.row_words(w, h)), np.uint32), first, video.frame_rate, k)
    _save_array(output, rows)
    return {"frames": int(len(rows)), "first": first, "every": k}


def caption(rows, output, window=1.0, hold=0.5, gap=1, min_duration=1.0, min_width=3, max_height=0.25, fill=0.5, band=(0.0, 1.0), tracking=None):
    """Captions from a text file (CAPTION.md), on the host: a JSON list of {start, end, first, last, left, top, right, bottom, cells}, the
    box in pixels.  With `tracking` (what `track` wrote) every caption also lists the `tracks` on screen for at least half of it and
    whether one is `alone`.  The video is not opened.  Returns the list."""
    from . import text as _text
    table = _text.load(rows) if isinstance(rows, str) else _text.check(np.asarray(rows))
    tracks = _load(tracking, formats.read_tracks)
    found = _text.analyse(table, window=window, hold=hold, gap=gap, min_duration=min_duration, min_width=min_width, max_height=max_height,
                          fill=fill, band=band)
    listed = _text.report(table, found, tracks)
    _write_json(output, listed)
    return listed


def clothes(video, tracking, output, widen=0.5, drop=0.25, height=2.0, bands=2, min_size=0.0, keep_overlapped=False, t_from=0.0, t_until=None,
            batch=2048, ctx=None, ahead=96):
    """What every track wears (CLOTHES.md): one pass over the frames that carry faces, as `talk` makes it without the carried frame.  The
    torso windows (clothes.torso) of the faces whose time lies in [t_from, t_until) go through Context.frame_hist in calls of `batch`
    windows, one group per track present in the call; the uint32 results are added into an int64 table on the host, so the file does
    not depend on `batch`.  Writes int64 [T][6 + 256 bands], a row per track of the tracking file in ascending track number: track, ms
    of its first and last row in the range (-1 without one), faces used, faces skipped, bands, the histogram.  Returns {"tracks",
    "faces", "skipped"}."""
    from . import clothes as _clothes, runtime
    from .feed import FrameFeed
    from .pipeline import faces_per_frame
    from .talk import ms
    if not 1 <= int(batch) <= _clothes.MAX_WINDOWS:
        raise ValueError("clothes: a batch holds 1 .. %d windows" % _clothes.MAX_WINDOWS)
    if not 1 <= int(bands) <= _clothes.MAX_BANDS:
        raise ValueError("clothes: --bands is 1 .. %d" % _clothes.MAX_BANDS)
    if widen < 0 or drop < 0 or height < 0 or min_size < 0:
        raise ValueError("clothes: --widen, --drop, --height and --min-size are not negative")
    bands, batch = int(bands), int(batch)
    W, H = video.frame_size
    rows = _load(tracking, formats.read_tracks)
    tracks = sorted(set(int(r[1]) for r in rows))
    row_of = dict((t, k) for k, t in enumerate(tracks))
    table = np.zeros((len(tracks), _clothes.HEAD + _clothes.BINS * bands), np.int64)
    table[:, 0], table[:, 1], table[:, 2], table[:, 5] = tracks, -1, -1, bands
    by_frame = {}                            # frame index -> [(track, window)] of the faces that count
    for fi, T, faces in faces_per_frame(rows, _frame_times(video, rows), W, H, drop_last=False):
        if T < t_from or (t_until is not None and not T < t_until):
            continue
        faces = [(int(t), b) for t, b in faces]
        for (t, _), win in zip(faces, _clothes.windows_of(faces, W, H, widen, drop, height, min_size, keep_overlapped)):
            r = table[row_of[t]]
            r[1], r[2] = (ms(T) if r[1] < 0 else min(r[1], ms(T))), max(r[2], ms(T))
            if win is None:
                r[4] += 1
            else:
                r[3] += 1
                by_frame.setdefault(fi, []).append((t, win))
    if by_frame:
        ctx = ctx or runtime.default_context()
        with FrameFeed(ctx, video, by_frame, ahead=ahead, name="pvface-clothes-reader") as feed:
            jobs, held = [], []              # [(device frame, track, window)] waiting for a call; [[device frame, its windows still waiting]]

            def call(k):
                part = jobs[:k]
                del jobs[:k]
                _clothes.measure(ctx, [j[0] for j in part], [j[2] for j in part], [j[1] for j in part], bands, table, row_of)
                while k:                     # a frame goes when its last window has been measured
                    took = min(k, held[0][1])
                    held[0][1] -= took
                    k -= took
                    if not held[0][1]:
                        feed.release(held.pop(0)[0])
            for fi, dev in feed:
                held.append([dev, len(by_frame[fi])])
                jobs.extend((dev, t, win) for t, win in by_frame[fi])
                while len(jobs) >= batch:
                    call(batch)
            if jobs:
                call(len(jobs))
    _save_array(output, table)
    return {"tracks": len(tracks), "faces": int(table[:, 3].sum()), "skipped": int(table[:, 4].sum())}


def link(table, output, min_score=0.75, margin=0.05, max_gap=120.0, min_faces=3, min_pixels=20000, labels=None, merged=None):
    """Which tracks wear the same clothes (CLOTHES.md "Link"), on the host, from a clothes file alone: JSON {"parameters", "links":
    [{"a", "b", "score"}]} with a < b, sorted.  With `labels` and `merged` the `identifier name` file of `cluster` or `identify` is
    written again with the clusters merged along the links.  The pair scores are numpy on the host: a film has a few thousand tracks.
    Returns the links."""
    from . import clothes as _clothes, render
    if (labels is None) != (merged is None):
        raise ValueError("link: --labels and --merged come together")
    t = _clothes.load(table) if isinstance(table, str) else _clothes.check(np.asarray(table))
    found = _clothes.links(t, min_score=min_score, margin=margin, max_gap=max_gap, min_faces=min_faces, min_pixels=min_pixels)
    doc = {"parameters": {"min_score": _clothes.fraction(min_score, "min-score"), "margin": _clothes.fraction(margin, "margin"),
                          "max_gap_ms": _clothes.ms(max_gap), "min_faces": int(min_faces), "min_pixels": int(min_pixels)},
           "links": [{"a": a, "b": b, "score": s} for a, b, s in found]}
    _write_json(output, doc)
    if labels is not None:
        names = _clothes.merge_labels(_load(labels, render.read_labels), found, t)
        with open(merged, "w") as fo:
            for identifier in sorted(names):
                fo.write("%d %s\n" % (identifier, names[identifier]))
    return doc["links"]


def demo(video, tracking, output, height=400, t_from=0.0, t_until=None, shift=0.0, landmark=None, label=None, matrix="601",
         full_range=False, fps=None, ctx=None, ring_depth=16):
    """Annotated video (pyannote-face.py:317-413) as YUV4MPEG2, to a path or to stdout (`-`).  What is drawn on which frame is planned
    on the host (render.build_plan: the pacing of getFaceGenerator / getLandmarkGenerator); a reader thread pushes the frames the plan
    shows through the pinned ingest ring (RGB or YUV, as `track` does), this thread submits one render per output frame to the egress
    ring, a writer thread waits for the slots and writes them: rendering frame k + 1 overlaps the copy of frame k and the write of
    frame k - 1.  Audio is not carried.  Returns {"frames": output frames, "width", "height"}."""
    from . import render, runtime
    ctx = ctx or runtime.default_context()
    vw, vh = video.size
    width, height = render.demo_size(vw, vh, height)
    rate = float(video.frame_rate)
    labels, marks, rows = _load(label, render.read_labels), _load(landmark, formats.read_landmarks), _load(tracking, formats.read_tracks)
    plan = render.build_plan(rows, rate, len(video), width, height, marks, labels, t_from, t_until, shift)
    return _render_plan(video, plan, output, width, height, matrix, full_range, fps if fps is not None else rate, ctx, ring_depth)


def _render_plan(video, plan, output, width, height, matrix, full_range, fps, ctx, ring_depth):
    """What `demo` and `redact` share: the frames a plan of (source index, t, primitives) shows go reader thread -> pinned ingest ring ->
    one render per output frame into the egress ring (this thread) -> writer thread -> YUV4MPEG2."""
    import queue
    import threading
    from . import render
    from .feed import FrameFeed
    by_index = {}
    for k, (i, _, _) in enumerate(plan):
        by_index.setdefault(i, []).append(k)
    ring = ctx.egress_ring(width, height, matrix, full_range, depth=ring_depth)
    writer = render.Y4mWriter(output, width, height, render.rate_tag(video, fps), full_range)
    wq = queue.Queue()
    free = threading.Semaphore(ring_depth)             # slots the writer has given back
    state = {"error": None}                            # the writer thread's; an error of this thread stops its writes

    def drain():
        try:
            while True:
                slot = wq.get()
                if slot is None:
                    return
                if state["error"] is None:
                    writer.write(ring.wait(slot))
                    ring.release(slot)
                free.release()
        except BaseException as e:          # noqa: BLE001 -- re-raised below
            state["error"] = e
            free.release()
            while wq.get() is not None:
                free.release()

    wt = threading.Thread(target=drain, name="pvface-demo-writer")
    try:
        with FrameFeed(ctx, video, by_index, ahead=ring_depth, ring_depth=ring_depth, seek=True, name="pvface-demo-reader") as feed:
            wt.start()
            try:
                for fi, dev in feed:
                    if state["error"] is not None:
                        break
                    for k in by_index[fi]:
                        free.acquire()
                        if state["error"] is not None:
                            free.release()
                            break
                        wq.put(ring.submit(dev, plan[k][2]))
                    feed.release(dev)            # the kernels that read it are queued: the buffer is recycled behind them
            except BaseException as e:          # noqa: BLE001 -- on its way to the caller
                state["error"] = state["error"] or e
                raise
            finally:
                wq.put(None)
                wt.join()
    finally:
        writer.close()
        ring.close()
    if state["error"] is not None:
        raise state["error"]
    return {"frames": writer.frames, "width": width, "height": height}


def redact(video, tracking, output, height=0, t_from=0.0, t_until=None, shift=0.0, label=None, only=None, keep=None, pad=25, cells=8,
           shape="ellipse", mode="mosaic", colour=(0, 0, 0), draw=False, matrix="601", full_range=False, fps=None, ctx=None, ring_depth=16):
    """The video with the faces of the chosen tracks hidden (REDACT.md), as YUV4MPEG2 to a path or to stdout (`-`): pixelated
    (`mosaic`), pixelated and blended (`smooth`) or filled with `colour`.  height 0 keeps the source size.  only / keep: label names
    (render.build_redaction_plan's selection); draw: `demo`'s primitives on top of the redactions.  It hides what the tracking file
    holds: a face the detector never found stays visible.  Returns {"frames", "width", "height", "redactions"}."""
    from . import render, runtime
    ctx = ctx or runtime.default_context()
    vw, vh = video.size
    width, height = (int(vw), int(vh)) if not height else render.demo_size(vw, vh, height)
    rate = float(video.frame_rate)
    labels, rows = _load(label, render.read_labels), _load(tracking, formats.read_tracks)
    plan = render.build_redaction_plan(rows, rate, len(video), width, height, labels, only, keep, pad, cells, shape, mode, colour,
                                       t_from, t_until, shift)
    count = sum(len(prims) for _, _, prims in plan)
    if draw:
        drawn = render.build_plan(rows, rate, len(video), width, height, None, labels, t_from, t_until, shift)
        plan = [(i, t, prims + more) for (i, t, prims), (_, _, more) in zip(plan, drawn)]
    res = _render_plan(video, plan, output, width, height, matrix, full_range, fps if fps is not None else rate, ctx, ring_depth)
    res["redactions"] = count
    return res


def faces(video, tracking, landmarks, output, per=4, tile=150, columns=None, label=None, only=None, spread=1.0, min_size=0.0, max_dark=0.25,
          max_bright=0.25, t_from=0.0, t_until=None, index=None, quality=None, ctx=None, batch=2048, ahead=96):
    """The contact sheet of the best faces of every track, or with `label` of every cluster or name (FACES.md).  Two passes over the
    video.  Pass 1 is `extract`'s loop: a reader thread pushes the frames that carry faces through the pinned ingest ring, this thread
    asks for the quality sums of `batch` faces per library call (the chips are made and reduced on the device; 40 bytes a face come
    back).  The choice is made here (faces.py).  Pass 2 reads only the frames of the chosen faces and makes one sheet call.  Returns
    {"width", "height", "groups", "faces", "shown"}."""
    from . import faces as _faces, render, runtime
    from .feed import FrameFeed
    ctx = ctx or runtime.default_context()
    _check_sheet_name("faces", output)
    if not _faces.MIN_TILE <= int(tile) <= _faces.MAX_TILE:
        raise ValueError("faces: --tile is %d .. %d" % (_faces.MIN_TILE, _faces.MAX_TILE))
    if int(per) < 1:
        raise ValueError("faces: --per is at least 1")
    frame_width, frame_height = video.frame_size
    rows, marks, labels = _load(tracking, formats.read_tracks), _load(landmarks, formats.read_landmarks), _load(label, render.read_labels)
    all_faces = _faces.landmark_faces(rows, marks, _frame_times(video, rows), frame_width, frame_height)
    by_frame = {}
    for i, f in enumerate(all_faces):
        by_frame.setdefault(f[2], []).append(i)
    sums = np.zeros((len(all_faces), 5), np.int64)

    # ---- pass 1: the quality of every face
    with FrameFeed(ctx, video, by_frame, ahead=ahead, name="pvface-faces-reader") as feed:
        for part in feed.batches(batch, lambda fi: len(by_frame[fi])):
            jobs = [(dev, i) for fi, dev in part for i in by_frame[fi]]
            idx = [i for _, i in jobs]
            sums[idx] = ctx.face_quality([dev for dev, _ in jobs], np.stack([all_faces[i][4] for i in idx]))
            feed.release_all(dev for _, dev in part)

    # ---- the choice
    sym = [_faces.symmetry(f[4]) for f in all_faces]
    sc = [_faces.score(sums[i], sym[i]) for i in range(len(all_faces))]
    ok = [_faces.eligible(sums[i], f[3][3] - f[3][1], frame_height, max_dark, max_bright, min_size) for i, f in enumerate(all_faces)]
    if quality:
        with open(quality, "w") as fq:
            for i, f in enumerate(all_faces):
                fq.write(_faces.quality_line(f[0], f[1], sums[i], sym[i], sc[i], ok[i]))
    groups = _faces.group_faces(all_faces, labels, only, t_from, t_until)
    if not groups:
        raise ValueError("faces: no face to show (an empty landmark file, or --only / --from / --until leave none)")
    shown = []
    for name, colour, idx in groups:
        pick = _faces.choose([(sc[i], all_faces[i][0], all_faces[i][1], ok[i]) for i in idx], int(per), spread)
        shown.append([idx[k] for k in pick])
    cols = int(columns) if columns else _faces.default_columns(len(groups))
    W, H, corners, prims = _faces.layout([(g[0], g[1], len(s)) for g, s in zip(groups, shown)], int(per), int(tile), cols)
    flat = [i for s in shown for i in s]
    _faces.check_sheet(W, H, len(flat), len(prims))
    if index:
        with open(index, "w") as fx:
            for g, s in zip(groups, shown):
                for rank, i in enumerate(s):
                    fx.write("%s %d " % (g[0], rank) + _faces.quality_line(all_faces[i][0], all_faces[i][1], sums[i], sym[i], sc[i], ok[i]))

    # ---- pass 2: the frames of the chosen faces, one sheet call
    need = set(all_faces[i][2] for i in flat)
    with FrameFeed(ctx, video, need, ahead=ahead, ring_depth=max(2, min(len(need), 16)), seek=True, name="pvface-faces-reader") as feed:
        dev = dict(feed)
        sheet = ctx.face_sheet([dev[all_faces[i][2]] for i in flat], np.stack([all_faces[i][4] for i in flat]),
                               [xy for c in corners for xy in c], int(tile), W, H, _faces.BACKGROUND, prims)
    _write_sheet(output, sheet)
    return {"width": W, "height": H, "groups": [g[0] for g in groups], "faces": len(all_faces), "shown": len(flat)}


def talk(video, tracking, landmarks, output, window=0.4, on=3.0, off=1.5, min_duration=0.3, max_pause=0.3, max_dark=0.25, t_from=0.0,
         t_until=None, label=None, segments=None, ctx=None, batch=2048, ahead=96):
    """Lip activity of every face and the spans in which a track is taken to be talking (TALK.md).  One pass over the video, pass 1 of
    `faces`: a reader thread pushes the frames that carry faces through the pinned ingest ring, this thread asks for the eight motion
    integers of a batch of whole frames per library call (chips, patches and sums are made on the device; 32 bytes a face come back).
    A face is compared with the face of its track on the frame before; the last frame of a batch is kept alive and leads the next
    call, its faces without a predecessor and their rows discarded, so links cross batches.  The rest is talk.py.  Returns {"faces",
    "linked", "segments"}."""
    from . import faces as _faces, render, runtime, talk as _talk
    from .feed import FrameFeed
    ctx = ctx or runtime.default_context()
    if int(batch) < 1:
        raise ValueError("talk: a batch holds at least one face")
    frame_width, frame_height = video.frame_size
    rows, marks, labels = _load(tracking, formats.read_tracks), _load(landmarks, formats.read_landmarks), _load(label, render.read_labels)
    all_faces = [f for f in _faces.landmark_faces(rows, marks, _frame_times(video, rows), frame_width, frame_height)
                 if f[0] >= t_from and (t_until is None or f[0] < t_until)]
    prev = _talk.link([(f[2], f[1]) for f in all_faces])
    by_frame = {}
    for i, f in enumerate(all_faces):
        by_frame.setdefault(f[2], []).append(i)
    out = np.full((len(all_faces), 8), -1, np.int32)

    with FrameFeed(ctx, video, by_frame, ahead=ahead, name="pvface-talk-reader") as feed:
        carry = []                           # [(frame index, device frame)]: the last frame of the batch before
        for part in feed.batches(batch, lambda fi: len(by_frame[fi])):
            frames, idx = [], []
            for fi, dev in carry + part:
                for i in by_frame[fi]:
                    frames.append(dev); idx.append(i)
            lead = sum(len(by_frame[fi]) for fi, _ in carry)
            local = dict((i, k) for k, i in enumerate(idx))
            p = [-1 if k < lead else local.get(prev[i], -1) for k, i in enumerate(idx)]
            got = ctx.face_motion(frames, np.stack([all_faces[i][4] for i in idx]), p)
            out[idx[lead:]] = got[lead:]
            feed.release_all(dev for _, dev in carry + part[:-1])
            carry = part[-1:]

    linked = [p >= 0 for p in prev]
    per, segs = _talk.analyse([(f[0], f[1], f[4]) for f in all_faces], out, linked, window, on, off, min_duration, max_pause, max_dark)
    text = "".join(_talk.face_line(f[0], f[1], out[i], *per[i]) for i, f in enumerate(all_faces))
    if str(output) == "-":
        sys.stdout.write(text)
        sys.stdout.flush()
    else:
        with open(output, "w") as fo:
            fo.write(text)
    if segments:
        with open(segments, "w") as fs:
            for track, start, end, mean in segs:
                fs.write(_talk.segment_line(track, start, end, mean, None if labels is None else (labels.get(track) or "#%d" % track)))
    return {"faces": len(all_faces), "linked": int(sum(linked)), "segments": segs}


def tube(video, tracking, landmarks, output, size=224, region="face", scale=None, smooth=0.5, label=None, only=None, segments=None,
         min_length=0.0, t_from=0.0, t_until=None, fmt="y4m", matrix="601", full_range=False, index=None, fps=25.0, ctx=None, batch=2048,
         ahead=96, max_open=None, align=False):
    """A fixed-size face or mouth video for every track (TUBE.md).  One pass over the video, shaped like `talk`'s: a reader thread pushes
    the frames that carry chosen faces through the pinned ingest ring, this thread asks for `batch` pictures per library call (the
    windows are resampled, and for Y4M converted, on the device from the resident frames; only the pictures come back) and appends
    each to the file of its tube.  The windows are made before the pass (tube.py), so every file's length is known when it is opened;
    at most `max_open` files are open at a time (tube.FilePool).  With `align` the windows follow the smoothed eye line of the landmarks
    (oriented windows, Context.frame_warps) and the index lines carry `CX CY BX BY K`.  Returns {"tubes", "pictures", "files", "open_peak"}."""
    import os
    from . import faces as _faces, pipeline, render, runtime, tube as _tube
    from .feed import FrameFeed
    ctx = ctx or runtime.default_context()
    if fmt not in ("y4m", "npy"):
        raise ValueError("tube: the format is y4m or npy")
    if region == "mouth" and landmarks is None:
        raise ValueError("tube: --region mouth needs the landmarks file of `extract` between the tracking file and the output directory")
    if align and landmarks is None:
        raise ValueError("tube: --align needs the landmarks file of `extract` between the tracking file and the output directory")
    if not _tube.MIN_SIZE <= int(size) <= _tube.MAX_SIZE:
        raise ValueError("tube: --size is %d .. %d" % (_tube.MIN_SIZE, _tube.MAX_SIZE))
    if int(batch) < 1 or int(batch) > _tube.MAX_CROPS:
        raise ValueError("tube: a batch holds 1 .. %d pictures" % _tube.MAX_CROPS)
    size = int(size)
    frame_width, frame_height = video.frame_size
    rows, labels, spans = _load(tracking, formats.read_tracks), _load(label, render.read_labels), _load(segments, _tube.read_segments)
    times = _frame_times(video, rows)
    if region == "mouth" or align:
        all_faces = _faces.landmark_faces(rows, _load(landmarks, formats.read_landmarks), times, frame_width, frame_height)
    if region == "face":                     # every face of the tracking file; aligned, with its points where the landmark file has a row for it
        points = dict(((int(round(f[0] * 1000.0)), f[1]), f[4]) for f in all_faces) if align else {}
        all_faces = [(T, int(ident), fi, box, points.get((int(round(T * 1000.0)), int(ident))))
                     for fi, T, g in pipeline.faces_per_frame(rows, times, frame_width, frame_height, drop_last=False) for ident, box in g]
    tubes = _tube.plan(all_faces, region, scale, smooth, labels, only, spans, min_length, t_from, t_until, fmt, align=bool(align), size=size)
    os.makedirs(output, exist_ok=True)
    by_frame = {}                            # frame index -> [(tube, picture, window)]
    for ti, (_, _, part) in enumerate(tubes):
        for k, (i, _, win) in enumerate(part):
            by_frame.setdefault(all_faces[i][2], []).append((ti, k, win))
    pool = _tube.FilePool(_tube.MAX_OPEN if max_open is None else max_open)
    writers, left = {}, [len(part) for _, _, part in tubes]
    rate = render.rate_tag(video, fps)

    def write(ti, picture):
        if ti not in writers:
            target = _tube.PooledFile(pool, os.path.join(output, tubes[ti][0]))
            writers[ti] = (_tube.NpyWriter(target, left[ti], size) if fmt == "npy" else render.Y4mWriter(target, size, size, rate, full_range))
        writers[ti].write(picture)
        left[ti] -= 1
        if not left[ti]:
            writers.pop(ti).close()

    try:
        with FrameFeed(ctx, video, by_frame, ahead=ahead, name="pvface-tube-reader") as feed:
            for part in feed.batches(batch, lambda fi: len(by_frame[fi])):
                jobs = [(dev, job) for fi, dev in part for job in by_frame[fi]]
                for k0 in range(0, len(jobs), int(batch)):
                    call = jobs[k0:k0 + int(batch)]
                    got = (ctx.frame_warps if align else ctx.frame_crops)([dev for dev, _ in call], [job[2] for _, job in call], size,
                                                                          "rgb" if fmt == "npy" else "yuv420", matrix, full_range)
                    for (_, (ti, _, _)), picture in zip(call, got):
                        write(ti, picture)
                feed.release_all(dev for _, dev in part)
    finally:
        for wr in writers.values():
            wr.close()
        pool.close()
    if index:
        with open(index, "w") as fx:
            for fname, track, part in tubes:
                for k, (_, T, win) in enumerate(part):
                    fx.write(_tube.index_line(fname, k, T, track, win))
    return {"tubes": len(tubes), "pictures": sum(len(part) for _, _, part in tubes), "files": [t[0] for t in tubes], "open_peak": pool.peak}


def _names(text):
    return set(n for n in text.split(",") if n)


def _colour(text):
    c = tuple(int(v) for v in text.split(","))
    if len(c) != 3 or not all(0 <= v <= 255 for v in c):
        raise argparse.ArgumentTypeError("a colour is r,g,b with each 0 .. 255")
    return c


def _parser():
    ap = argparse.ArgumentParser(prog="pyannote-face", description="face tracking => feature extraction => face clustering (MI355X)")
    ap.add_argument("--fps", type=float, default=25.0, help="frame rate of a .npy / synthetic video (Y4M: only if its header names none)")
    ap.add_argument("--matrix", choices=("601", "709"), default=None, help="YUV matrix of a Y4M video (its header cannot name one; default BT.601)")
    ap.add_argument("--range", choices=("limited", "full"), default=None, help="sample range of a Y4M video (default: XCOLORRANGE of its "
                    "header, else limited)")
    ap.add_argument("--device", type=int, default=None, help="GPU index (default: LOCAL_RANK or 0)")
    ap.add_argument("--metrics", default=None, help="write a JSON file with the run's timings and counts (frames, tracks, faces, seconds per stage, "
                    "frames resident at peak, device memory in use) next to the outputs")
    sub = ap.add_subparsers(dest="verb", required=True)
    t = sub.add_parser("track")
    t.add_argument("video"); t.add_argument("shot"); t.add_argument("tracking")
    t.add_argument("--min-size", type=float, default=0.0)
    t.add_argument("--every", type=float, default=0.0)
    t.add_argument("--min-overlap", type=float, default=MIN_OVERLAP_RATIO)
    t.add_argument("--min-confidence", type=float, default=MIN_CONFIDENCE)
    t.add_argument("--max-gap", type=float, default=MAX_GAP)
    e = sub.add_parser("extract")
    for name in ("video", "tracking", "landmark_model", "embedding_model", "landmarks", "embeddings"):
        e.add_argument(name)
    e.add_argument("--jitters", type=int, default=0, help="descriptors averaged over this many jittered face chips (dlib's num_jitters; "
                    "0 or 1: the plain descriptor)")
    e.add_argument("--jitter-seed", type=int, default=0, help="seed of the jitter transforms (they depend on the seed and the jitter's index alone)")
    pr = sub.add_parser("process", help="track + extract + cluster in one pass over the video")
    for name in ("video", "shot", "landmark_model", "embedding_model", "tracking", "landmarks", "embeddings"):
        pr.add_argument(name)
    pr.add_argument("--labels", default=None)
    pr.add_argument("--min-size", type=float, default=0.0)
    pr.add_argument("--every", type=float, default=0.0)
    pr.add_argument("--min-overlap", type=float, default=MIN_OVERLAP_RATIO)
    pr.add_argument("--min-confidence", type=float, default=MIN_CONFIDENCE)
    pr.add_argument("--max-gap", type=float, default=MAX_GAP)
    pr.add_argument("--threshold", type=float, default=0.6)
    pr.add_argument("--do-not-cooccur", action="store_true", help="tracks on screen at the same time never share a label")
    pr.add_argument("--gallery", default=None, help="a gallery file of `enroll`: matched clusters get names in the --labels file")
    pr.add_argument("--identify-threshold", type=float, default=0.6)
    pr.add_argument("--unknown", default=None, help="the name written for clusters nobody matches (default: their cluster number)")
    s = sub.add_parser("shot")
    s.add_argument("video"); s.add_argument("output")
    s.add_argument("--height", type=int, default=50, help="height of the images the optical flow runs on (reference default 50: one pyramid level; "
                   "64 and more bring OpenCV's coarser levels)")
    s.add_argument("--window", type=float, default=2.0)
    s.add_argument("--threshold", type=float, default=1.0)
    th = sub.add_parser("thread", help="shot threading (pyannote-structure.py thread)")
    th.add_argument("video"); th.add_argument("shot"); th.add_argument("output")
    th.add_argument("--min-match", type=int, default=20)
    th.add_argument("--lookahead", type=int, default=24)
    sc = sub.add_parser("scene", help="scenes from shot threads (pyannote-structure.py scene); the video is not opened")
    sc.add_argument("video"); sc.add_argument("thread"); sc.add_argument("output")
    sb = sub.add_parser("storyboard", help="the shots of a film as a contact sheet of thumbnails, as PPM or .npy")
    sb.add_argument("video"); sb.add_argument("shot"); sb.add_argument("output", help="a .ppm or .npy path, or - for a PPM on stdout")
    sb.add_argument("--per", type=int, default=1, choices=range(1, 9), metavar="1..8", help="frames shown per shot")
    sb.add_argument("--width", type=int, default=160, help="width of a thumbnail, 1 .. 1024; the height keeps the frame's aspect")
    sb.add_argument("--columns", type=int, default=None, help="shots per row (default: as many as 1920 pixels hold)")
    sb.add_argument("--thread", default=None, help="what `thread` or `scene` wrote: captions and outlines coloured by thread")
    sb.add_argument("--by", choices=("time", "thread"), default="time", help="shot order, or every thread on rows of its own")
    sb.add_argument("--from", dest="t_from", type=float, default=0.0, help="shots that start at or after this, seconds")
    sb.add_argument("--until", dest="t_until", type=float, default=None, help="shots that start before this, seconds")
    sb.add_argument("--index", default=None, help="write `shot k frame time x y label` per tile")
    sb.add_argument("--batch", type=int, default=64, help="frames reduced per library call, and resident at a time")
    fp = sub.add_parser("fingerprint", help="a 128-bit print of every frame of a video, as a uint64 [n][4] .npy file")
    fp.add_argument("video"); fp.add_argument("output", help="the .npy path the prints are written to")
    fp.add_argument("--from", dest="t_from", type=float, default=0.0, help="frames at or after this, seconds")
    fp.add_argument("--until", dest="t_until", type=float, default=None, help="frames before this, seconds")
    fp.add_argument("--batch", type=int, default=64, help="frames reduced per library call, and resident at a time")
    rp = sub.add_parser("repeat", help="the stretches print files of `fingerprint` share with themselves and with each other, as JSON")
    rp.add_argument("output", help="a path, or - for stdout")
    rp.add_argument("prints", nargs="+", help="print files; each is compared with itself and with every later one")
    rp.add_argument("--max-bits", type=int, default=10, help="bits of 128 in which two frames may differ and still match (0 .. 128)")
    rp.add_argument("--flat", type=int, default=16, help="a frame whose 9 x 9 luma spans less than this matches nothing (black, fades)")
    rp.add_argument("--min-duration", type=float, default=2.0, help="segments shorter than this are dropped, seconds")
    rp.add_argument("--max-gap", type=float, default=0.5, help="runs of one offset this close are one segment, seconds")
    rp.add_argument("--min-separation", type=float, default=5.0, help="within one file: only footage at least this far apart, seconds")
    bl = sub.add_parser("blend", help="the blend record of every frame of a video, as a uint32 [n][16] .npy file")
    bl.add_argument("video"); bl.add_argument("output", help="the .npy path the rows are written to")
    bl.add_argument("--width", type=int, default=64, help="width of the thumbnail that is measured; the height keeps the frame's aspect")
    bl.add_argument("--from", dest="t_from", type=float, default=0.0, help="frames at or after this, seconds")
    bl.add_argument("--until", dest="t_until", type=float, default=None, help="frames before this, seconds")
    bl.add_argument("--batch", type=int, default=64, help="frames measured per library call, and resident at a time")
    tr = sub.add_parser("transition", help="fades, dissolves and blank stretches from a blend file of `blend`, as JSON; the video is not opened")
    tr.add_argument("rows", help="the blend file"); tr.add_argument("output", help="a path, or - for stdout")
    tr.add_argument("--move", type=float, default=4.0, help="least mean change of luma over a window for it to count")
    tr.add_argument("--linear", type=float, default=0.25, help="largest share of that change the middle frame may lie off the line")
    tr.add_argument("--flat", type=float, default=2.0, help="a frame whose luma deviates less than this is blank")
    tr.add_argument("--min-duration", type=float, default=0.12, help="shorter spans and blank runs are dropped, seconds")
    tr.add_argument("--shots", default=None, help="what `shot` wrote: with --refined, the shots cut at the transitions")
    tr.add_argument("--refined", default=None, help="where the refined Timeline is written")
    tr.add_argument("--motion", default=None, help="what `motion` wrote for the same video: spans inside a pan, tilt or zoom are written as `camera`")
    mo = sub.add_parser("motion", help="the camera motion between every two consecutive frames of a video, as an int64 [n][10] .npy file")
    mo.add_argument("video"); mo.add_argument("output", help="the .npy path the rows are written to")
    mo.add_argument("--width", type=int, default=96, help="width of the small image the flow is computed on; the height keeps the frame's aspect")
    mo.add_argument("--from", dest="t_from", type=float, default=0.0, help="frames from this time on, seconds")
    mo.add_argument("--until", dest="t_until", type=float, default=None, help="frames before this, seconds")
    mo.add_argument("--batch", type=int, default=256, help="frames measured per library call, and resident at a time")
    ca = sub.add_parser("camera", help="pans, tilts, zooms and static stretches from a motion file of `motion`, as JSON; the video is not opened")
    ca.add_argument("rows", help="the motion file"); ca.add_argument("output", help="a path, or - for stdout")
    ca.add_argument("--pan", type=float, default=5.0, help="least pan or tilt, percent of the frame's side per second")
    ca.add_argument("--zoom", type=float, default=3.0, help="least zoom, percent of scale per second")
    ca.add_argument("--window", type=float, default=0.5, help="seconds the rates are averaged over, centred on the frame")
    ca.add_argument("--min-inliers", type=int, default=50, help="least share of a pair's pixels the model must hold, percent")
    ca.add_argument("--min-duration", type=float, default=0.5, help="shorter spans are dropped, seconds")
    ca.add_argument("--max-gap", type=float, default=0.2, help="runs of one label this close are one span, seconds")
    ca.add_argument("--shots", default=None, help="what `shot` wrote: pairs across a boundary do not count, spans do not cross one")
    tx = sub.add_parser("text", help="overlaid text per 16 x 16 cell of every frame at full resolution, as a uint32 [n][8 + ch wpr] .npy file")
    tx.add_argument("video"); tx.add_argument("output", help="the .npy path the rows are written to")
    tx.add_argument("--step", type=float, default=0.0, help="seconds between measured frames; 0: every frame")
    tx.add_argument("--edge", type=int, default=48, help="least horizontal luma difference of a stroke pixel, 1 .. 255")
    tx.add_argument("--still", type=int, default=8, help="largest luma change of a pixel that has not moved, 0 .. 254")
    tx.add_argument("--on", type=int, default=24, help="persistent stroke pixels that set a cell's bit, 1 .. 256")
    tx.add_argument("--from", dest="t_from", type=float, default=0.0, help="frames from this time on, seconds")
    tx.add_argument("--until", dest="t_until", type=float, default=None, help="frames before this, seconds")
    tx.add_argument("--batch", type=int, default=64, help="frames measured per library call, and resident at a time")
    cp = sub.add_parser("caption", help="name straps, subtitles and title cards from a text file of `text`, as JSON; the video is not opened")
    cp.add_argument("rows", help="the text file"); cp.add_argument("output", help="a path, or - for stdout")
    cp.add_argument("--window", type=float, default=1.0, help="seconds a cell is voted over, centred on the frame")
    cp.add_argument("--hold", type=float, default=0.5, help="least share of the window's frames with the cell's bit set, 0 .. 1")
    cp.add_argument("--gap", type=int, default=1, help="unheld cells between two held ones of a cell row that are closed: the spaces between words")
    cp.add_argument("--min-duration", type=float, default=1.0, help="shorter captions are dropped, seconds")
    cp.add_argument("--min-width", type=int, default=3, help="narrower captions are dropped, cells")
    cp.add_argument("--max-height", type=float, default=0.25, help="taller captions are dropped, share of the frame's height")
    cp.add_argument("--fill", type=float, default=0.5, help="least share of its box, over its frames, a caption fills, 0 .. 1")
    cp.add_argument("--rows", dest="band", default="0,1", help="A,B: only the cell rows whose centre lies in [A, B) of the frame's height")
    cp.add_argument("--tracking", default=None, help="what `track` wrote: the tracks on screen with each caption")
    cl = sub.add_parser("clothes", help="a colour histogram of the torso windows under the faces of every track, as an int64 [T][6 + 256 bands] .npy file")
    cl.add_argument("video"); cl.add_argument("tracking"); cl.add_argument("output", help="the .npy path the table is written to")
    cl.add_argument("--widen", type=float, default=0.5, help="face widths the window reaches beyond the face box on either side")
    cl.add_argument("--drop", type=float, default=0.25, help="face heights between the face box and the window's top")
    cl.add_argument("--height", type=float, default=2.0, help="face heights the window is tall")
    cl.add_argument("--bands", type=int, default=2, help="horizontal bands of the window with a histogram each, 1 .. 4")
    cl.add_argument("--min-size", type=float, default=0.0, help="smaller faces are skipped, share of the frame's height")
    cl.add_argument("--keep-overlapped", action="store_true", help="count windows that meet another track's face box too")
    cl.add_argument("--from", dest="t_from", type=float, default=0.0, help="faces from this time on, seconds")
    cl.add_argument("--until", dest="t_until", type=float, default=None, help="faces before this, seconds")
    cl.add_argument("--batch", type=int, default=2048, help="windows per library call")
    lk = sub.add_parser("link", help="the tracks that wear the same clothes, from a clothes file of `clothes`, as JSON; the video is not opened")
    lk.add_argument("table", help="the clothes file"); lk.add_argument("output", help="a path, or - for stdout")
    lk.add_argument("--min-score", type=float, default=0.75, help="least histogram intersection of a link, 0 .. 1")
    lk.add_argument("--margin", type=float, default=0.05, help="least lead of a track's best candidate over its second best, 0 .. 1")
    lk.add_argument("--max-gap", type=float, default=120.0, help="largest time between the two tracks, seconds")
    lk.add_argument("--min-faces", type=int, default=3, help="tracks with fewer counted faces take no part")
    lk.add_argument("--min-pixels", type=int, default=20000, help="tracks with fewer counted pixels take no part")
    lk.add_argument("--labels", default=None, help="`identifier name` lines of `cluster` or `identify`: merged along the links into --merged")
    lk.add_argument("--merged", default=None, help="the label file written with --labels")
    c = sub.add_parser("cluster")
    c.add_argument("embeddings"); c.add_argument("labels")
    c.add_argument("--threshold", type=float, default=0.6)
    c.add_argument("--force", action="store_true")
    c.add_argument("--metric", choices=("euclidean", "cosine"), default="euclidean")
    c.add_argument("--do-not-cooccur", action="store_true", help="tracks on screen at the same time never share a label "
                   "(the constraint face/clustering.py:142 names and leaves off)")
    i = sub.add_parser("identify", help="names for tracks (or, with --labels, clusters) against a gallery of enrolled faces")
    i.add_argument("embeddings"); i.add_argument("gallery"); i.add_argument("output")
    i.add_argument("--threshold", type=float, default=0.6, help="largest mean pairwise distance that is still the same person")
    i.add_argument("--metric", choices=("euclidean", "cosine"), default="euclidean")
    i.add_argument("--labels", default=None, help="`identifier label` lines of `cluster`: decide per cluster, write a complete replacement")
    i.add_argument("--unknown", default=None, help="the name written where nobody matches")
    i.add_argument("--scores", default=None, help="write `group best_name best_dist second_name second_dist` per group")
    en = sub.add_parser("enroll", help="the largest face of every frame of a video, under a name, into a gallery file")
    for name in ("video", "landmark_model", "embedding_model", "name", "gallery"):
        en.add_argument(name)
    en.add_argument("--append", action="store_true", help="add to an existing gallery file (refused otherwise)")
    en.add_argument("--jitters", type=int, default=0, help="descriptors averaged over this many jittered face chips (dlib's num_jitters; "
                    "0 or 1: the plain descriptor)")
    en.add_argument("--jitter-seed", type=int, default=0, help="seed of the jitter transforms (they depend on the seed and the jitter's index alone)")
    ca = sub.add_parser("cast", help="the persons of one or more embedding files: rank-order clustering on the exact k-NN graph")
    ca.add_argument("output", help="a path, or - for stdout: `path track person` lines")
    ca.add_argument("embeddings", nargs="+", help="the embedding files whose tracks are grouped into persons")
    ca.add_argument("-k", type=int, default=64, help="neighbours per node (1 .. 256)")
    ca.add_argument("--max-distance", type=float, default=0.6, help="no neighbour further than this")
    ca.add_argument("--threshold", type=float, default=2.0, help="a pair is linked when its missing neighbours are at most this many per rank")
    ca.add_argument("--by", default="track", help="track: one node per (file, track), its mean descriptor; face: one node per row")
    ca.add_argument("--labels", default=None, metavar="SUFFIX", help="also write <embeddings>SUFFIX beside each file: `identifier label` lines")
    ca.add_argument("--graph", default=None, metavar="PATH", help="also write the k-NN lists and the node table as an .npz")
    se = sub.add_parser("search", help="the exact k nearest faces of one or more embedding files to a track or to a person of a gallery")
    se.add_argument("output", help="a path, or - for stdout: `rank distance path track T` lines, nearest first")
    se.add_argument("embeddings", nargs="+", help="the embedding files that are searched")
    se.add_argument("-k", type=int, default=100, help="faces kept (1 .. 1024)")
    se.add_argument("--max-distance", type=float, default=None, help="no face further than this (0.6: the same person, by the embedder's convention)")
    se.add_argument("--rows", action="store_true", help="every one of the k faces, not the best of each (file, track) among them")
    se.add_argument("--include-self", action="store_true", help="with --from: the query's own track may be found")
    se.add_argument("--gallery", default=None); se.add_argument("--name", default=None)
    se.add_argument("--from", dest="source", default=None, help="the embedding file the query track is taken from")
    se.add_argument("--track", type=int, default=None)
    et = sub.add_parser("enroll-track", help="the rows of one track of an embedding file, under a name, into a gallery file")
    et.add_argument("embeddings"); et.add_argument("track", type=int); et.add_argument("name"); et.add_argument("gallery")
    et.add_argument("--append", action="store_true")
    d = sub.add_parser("demo", help="the video with tracks, labels and landmarks drawn on it, as YUV4MPEG2")
    d.add_argument("video"); d.add_argument("tracking"); d.add_argument("output", help="a .y4m path, or - for stdout")
    d.add_argument("--height", type=int, default=400, help="height of the output frames; the width keeps the aspect")
    d.add_argument("--from", dest="t_from", type=float, default=0.0, help="start, seconds")
    d.add_argument("--until", dest="t_until", type=float, default=None, help="end, seconds (default: the video's duration)")
    d.add_argument("--shift", type=float, default=0.0, help="shift the tracks by this many seconds")
    d.add_argument("--landmark", default=None, help="landmarks.txt of `extract`: draws the nose line")
    d.add_argument("--label", default=None, help="`identifier label` lines, what `cluster` writes")
    rd = sub.add_parser("redact", help="the video with the faces of chosen tracks pixelated or filled, as YUV4MPEG2")
    rd.add_argument("video"); rd.add_argument("tracking"); rd.add_argument("output", help="a .y4m path, or - for stdout")
    rd.add_argument("--height", type=int, default=0, help="height of the output frames (0, the default: the source size)")
    rd.add_argument("--from", dest="t_from", type=float, default=0.0, help="start, seconds")
    rd.add_argument("--until", dest="t_until", type=float, default=None, help="end, seconds (default: the video's duration)")
    rd.add_argument("--shift", type=float, default=0.0, help="shift the tracks by this many seconds")
    rd.add_argument("--label", default=None, help="`identifier name` lines, what `cluster` and `identify` write")
    which = rd.add_mutually_exclusive_group()
    which.add_argument("--only", type=_names, default=None, metavar="A,B", help="redact only the tracks with these labels (needs --label)")
    which.add_argument("--keep", type=_names, default=None, metavar="A,B", help="redact every track but those with these labels; a track "
                       "without a label is redacted (needs --label)")
    rd.add_argument("--pad", type=int, default=25, help="per cent of the box's width / height added on each side")
    rd.add_argument("--cells", type=int, default=8, help="mosaic cells along the longer side of the padded box")
    rd.add_argument("--shape", choices=("ellipse", "box"), default="ellipse")
    rd.add_argument("--mode", choices=("mosaic", "smooth", "fill"), default="mosaic")
    rd.add_argument("--colour", type=_colour, default=(0, 0, 0), metavar="r,g,b", help="the fill colour")
    rd.add_argument("--draw", action="store_true", help="draw what `demo` draws on top of the redactions")
    fc = sub.add_parser("faces", help="a contact sheet of the best faces of every track, cluster or name, as PPM or .npy")
    fc.add_argument("video"); fc.add_argument("tracking"); fc.add_argument("landmarks", help="landmarks.txt of `extract`")
    fc.add_argument("output", help="a .ppm or .npy path, or - for a PPM on stdout")
    fc.add_argument("--per", type=int, default=4, help="faces shown per group")
    fc.add_argument("--tile", type=int, default=150, help="side of a face on the sheet, 48 .. 600 (150: the aligned chip itself)")
    fc.add_argument("--columns", type=int, default=None, help="panels per row (default: 1 up to 24 groups, then ceil(groups / 24))")
    fc.add_argument("--label", default=None, help="`identifier name` lines, what `cluster` and `identify` write: a group per name")
    fc.add_argument("--only", type=_names, default=None, metavar="A,B", help="show only these groups (names; #7 or 7 for a track)")
    fc.add_argument("--spread", type=float, default=1.0, help="seconds between two shown faces of one track, while others are left")
    fc.add_argument("--min-size", type=float, default=0.0, help="smallest box height, as a share of the frame height, of an eligible face")
    fc.add_argument("--max-dark", type=float, default=0.25, help="largest share of pixels with luma <= 16 of an eligible face")
    fc.add_argument("--max-bright", type=float, default=0.25, help="largest share of pixels with luma >= 239 of an eligible face")
    fc.add_argument("--from", dest="t_from", type=float, default=0.0, help="start, seconds")
    fc.add_argument("--until", dest="t_until", type=float, default=None, help="end, seconds (default: the video's duration)")
    fc.add_argument("--index", default=None, help="write `group rank T track S1 S2 SY ND NB sym score eligible` per shown face")
    fc.add_argument("--quality", default=None, help="write `T track S1 S2 SY ND NB sym score eligible` for every face of the film")
    tk = sub.add_parser("talk", help="lip activity of every face and the spans in which a track is taken to be talking")
    tk.add_argument("video"); tk.add_argument("tracking"); tk.add_argument("landmarks", help="landmarks.txt of `extract`")
    tk.add_argument("output", help="`T track DM0 DMmin kM DC0 DCmin kC SM NZ open a s talking` per face; - for stdout")
    tk.add_argument("--window", type=float, default=0.4, help="seconds the activity is averaged over, centred on the face")
    tk.add_argument("--on", type=float, default=3.0, help="smoothed activity (grey levels per pixel) at which talking turns on")
    tk.add_argument("--off", type=float, default=1.5, help="smoothed activity below which talking turns off")
    tk.add_argument("--min-duration", type=float, default=0.3, help="spans shorter than this many seconds are dropped")
    tk.add_argument("--max-pause", type=float, default=0.3, help="spans of a track no more than this many seconds apart are merged")
    tk.add_argument("--max-dark", type=float, default=0.25, help="largest share of window pixels with luma <= 16 of a valid face")
    tk.add_argument("--from", dest="t_from", type=float, default=0.0, help="start, seconds")
    tk.add_argument("--until", dest="t_until", type=float, default=None, help="end, seconds (default: the video's duration)")
    tk.add_argument("--label", default=None, help="`identifier name` lines: --segments lines end in the track's name")
    tk.add_argument("--segments", default=None, help="write `track start end mean_s` per talking span")
    tb = sub.add_parser("tube", help="a fixed-size face or mouth video for every track, as YUV4MPEG2 or .npy files in a directory")
    tb.add_argument("video"); tb.add_argument("tracking")
    tb.add_argument("rest", nargs="+", metavar="[landmarks] output-directory", help="landmarks.txt of `extract` (needed by --region mouth "
                    "and by --align), then the directory the tubes are written to")
    tb.add_argument("--size", type=int, default=224, help="side of the pictures, 1 .. 1024")
    tb.add_argument("--region", choices=("face", "mouth"), default="face")
    tb.add_argument("--scale", type=float, default=None, help="face: the window's side over the larger side of the track box (default 1.6); "
                    "mouth: over the same at scale 1 (default 0.5)")
    tb.add_argument("--smooth", type=float, default=0.5, help="seconds the window's centre and side are averaged over (0: the raw values)")
    tb.add_argument("--label", default=None, help="`identifier name` lines, what `cluster` and `identify` write")
    tb.add_argument("--only", type=_names, default=None, metavar="A,B", help="only the tracks with these names (#7 or 7 for a track)")
    tb.add_argument("--segments", default=None, help="the file `talk --segments` wrote: one tube per span, track_%%05d_%%03d")
    tb.add_argument("--min-length", type=float, default=0.0, help="tubes shorter than this many seconds are dropped")
    tb.add_argument("--from", dest="t_from", type=float, default=0.0, help="start, seconds")
    tb.add_argument("--until", dest="t_until", type=float, default=None, help="end, seconds (default: the video's duration)")
    tb.add_argument("--format", dest="fmt", choices=("y4m", "npy"), default="y4m")
    tb.add_argument("--matrix", dest="out_matrix", choices=("601", "709"), default=None, help="YUV matrix of the Y4M tubes (default: the video's, else 601)")
    tb.add_argument("--range", dest="out_range", choices=("limited", "full"), default=None, help="sample range of the Y4M tubes")
    tb.add_argument("--align", action="store_true", help="roll-aligned tubes: the windows are turned so that the eye line of the landmarks, "
                    "smoothed like the centre, is horizontal (needs the landmarks file)")
    tb.add_argument("--index", default=None, help="write `file picture T track X0 Y0 L` per picture (with --align: `... track CX CY BX BY K`)")
    return ap


def parse_args(argv=None):
    return _parser().parse_args(argv)


# the refusals of a verb that are the user's to mend, and so become usage errors (exit status 2) instead of tracebacks; a verb that is
# not listed lets every exception through
_REFUSALS = dict.fromkeys(("cast", "search", "storyboard", "repeat", "blend", "transition", "motion", "camera", "text", "caption", "clothes",
                           "link", "faces"), (ValueError,))
_REFUSALS.update(talk=(KeyError, ValueError), tube=(KeyError, ValueError))      # KeyError: a track or name the files do not hold


def main(argv=None):
    ap = _parser()
    a = ap.parse_args(argv)
    import time
    ctx = None
    if a.device is not None:
        from .runtime import Context
        ctx = Context(device=a.device)
    t_begin = time.perf_counter()
    refused = _REFUSALS.get(a.verb, ())
    try:
        res = _run(ap, a, ctx)
    except refused as e:
        ap.error(str(e.args[0]) if KeyError in refused and e.args else str(e))           # (a KeyError's own text wears quotes)
    if a.metrics:
        from . import runtime
        m = {"verb": a.verb, "seconds": round(time.perf_counter() - t_begin, 4)}
        if isinstance(res, dict):
            m.update(frames=res.get("frames"), tracks=len(res.get("tracks", ())), faces=int(len(res["face_T"])) if "face_T" in res else None,
                     clusters=len(set(res["labels"].values())) if res.get("labels") else None, peak_frames_resident=res.get("peak_frames_resident"),
                     stage_seconds={k: round(v, 4) for k, v in res.get("timings", {}).items()})
        try:
            free, total = (ctx or runtime.default_context()).mem_info()
            m["device_memory_in_use_bytes"] = total - free
        except Exception:          # noqa: BLE001 -- the figure is optional
            pass
        with open(a.metrics, "w") as f:
            json.dump(m, f, indent=1)
    return 0


def _run(ap, a, ctx):
    """the verb of the parsed arguments `a`: its argument checks, which refuse through ap.error, and its call -> what the verb returned"""
    res = None

    def video():
        if a.video == "-" and a.verb == "faces":
            ap.error("faces reads the video twice, once for the quality of every face and once for the frames of the chosen ones: "
                     "give it a file, not a stream on stdin")
        if a.video == "-" and a.verb not in ("track", "process", "talk", "tube", "fingerprint", "blend", "motion", "text", "clothes"):
            ap.error("%s needs the length of the video: give it a file, not a stream on stdin" % a.verb)
        over = {}
        if a.matrix is not None:
            over["matrix"] = a.matrix
        if a.range is not None:
            over["full_range"] = a.range == "full"
        return open_video(a.video, a.fps, **over)

    def colours(v, matrix, rng):
        """matrix and full_range of what a verb writes: the option, else what the video says of itself, else BT.601 limited"""
        return dict(matrix=matrix or getattr(v, "matrix", "601"),
                    full_range=(rng == "full") if rng is not None else bool(getattr(v, "full_range", False)))
    if a.verb == "track":
        res = track(video(), a.shot, a.tracking, detect_min_size=a.min_size, detect_every=a.every,
                    track_min_overlap_ratio=a.min_overlap, track_min_confidence=a.min_confidence, track_max_gap=a.max_gap, ctx=ctx)
    elif a.verb == "process":
        if a.gallery is not None and a.labels is None:
            ap.error("--gallery names clusters: it needs --labels")
        res = process(video(), a.shot, a.landmark_model, a.embedding_model, a.tracking, a.landmarks, a.embeddings, a.labels,
                detect_min_size=a.min_size, detect_every=a.every, track_min_overlap_ratio=a.min_overlap,
                track_min_confidence=a.min_confidence, track_max_gap=a.max_gap, threshold=a.threshold, ctx=ctx, do_not_cooccur=a.do_not_cooccur,
                gallery=a.gallery, identify_threshold=a.identify_threshold, unknown=a.unknown)
    elif a.verb == "identify":
        identify(a.embeddings, a.gallery, a.output, threshold=a.threshold, metric=a.metric, labels=a.labels, unknown=a.unknown, scores=a.scores, ctx=ctx)
    elif a.verb == "enroll":
        res = enroll(video(), a.landmark_model, a.embedding_model, a.name, a.gallery, append=a.append, ctx=ctx, num_jitters=a.jitters,
                     jitter_seed=a.jitter_seed)
    elif a.verb == "enroll-track":
        enroll_track(a.embeddings, a.track, a.name, a.gallery, append=a.append)
    elif a.verb == "cast":
        cast(a.output, a.embeddings, k=a.k, max_distance=a.max_distance, threshold=a.threshold, by=a.by, labels=a.labels, graph=a.graph, ctx=ctx)
    elif a.verb == "search":
        search(a.output, a.embeddings, k=a.k, max_distance=a.max_distance, rows=a.rows, include_self=a.include_self, gallery=a.gallery,
               name=a.name, source=a.source, track=a.track, ctx=ctx)
    elif a.verb == "shot":
        shot(video(), a.output, height=a.height, window=a.window, threshold=a.threshold, ctx=ctx)
    elif a.verb == "thread":
        thread(video(), a.shot, a.output, min_match=a.min_match, lookahead=a.lookahead, ctx=ctx)
    elif a.verb == "scene":
        scene(a.video, a.thread, a.output)
    elif a.verb == "storyboard":
        if a.width < 1 or a.width > 1024 or a.batch < 1 or (a.columns is not None and a.columns < 1):
            ap.error("--width is 1 .. 1024, --batch and --columns at least 1")
        res = storyboard(video(), a.shot, a.output, per=a.per, width=a.width, columns=a.columns, thread=a.thread, by=a.by, t_from=a.t_from,
                         t_until=a.t_until, index=a.index, batch=a.batch, ctx=ctx)
    elif a.verb == "fingerprint":
        if a.batch < 1:
            ap.error("--batch is at least 1")
        res = fingerprint(video(), a.output, t_from=a.t_from, t_until=a.t_until, batch=a.batch, ctx=ctx)
    elif a.verb == "repeat":
        if not 0 <= a.max_bits <= 128:
            ap.error("--max-bits is 0 .. 128")
        repeat(a.output, a.prints, max_bits=a.max_bits, flat=a.flat, min_duration=a.min_duration, max_gap=a.max_gap,
               min_separation=a.min_separation, ctx=ctx)
    elif a.verb == "blend":
        if a.batch < 1 or a.width < 1:
            ap.error("--batch and --width are at least 1")
        res = blend(video(), a.output, width=a.width, t_from=a.t_from, t_until=a.t_until, batch=a.batch, ctx=ctx)
    elif a.verb == "transition":
        transition(a.rows, a.output, move=a.move, linear=a.linear, flat=a.flat, min_duration=a.min_duration, shots=a.shots, refined=a.refined,
                   motion=a.motion)
    elif a.verb == "motion":
        if a.batch < 1 or a.width < 1:
            ap.error("--batch and --width are at least 1")
        res = motion(video(), a.output, width=a.width, t_from=a.t_from, t_until=a.t_until, batch=a.batch, ctx=ctx)
    elif a.verb == "camera":
        camera(a.rows, a.output, pan=a.pan, zoom=a.zoom, window=a.window, min_inliers=a.min_inliers, min_duration=a.min_duration,
               max_gap=a.max_gap, shots=a.shots)
    elif a.verb == "text":
        res = text(video(), a.output, step=a.step, edge=a.edge, still=a.still, on=a.on, t_from=a.t_from, t_until=a.t_until, batch=a.batch, ctx=ctx)
    elif a.verb == "caption":
        band = tuple(float(v) for v in a.band.split(","))
        if len(band) != 2:
            raise ValueError("caption: --rows A,B with 0 <= A < B <= 1")
        caption(a.rows, a.output, window=a.window, hold=a.hold, gap=a.gap, min_duration=a.min_duration, min_width=a.min_width,
                max_height=a.max_height, fill=a.fill, band=band, tracking=a.tracking)
    elif a.verb == "clothes":
        res = clothes(video(), a.tracking, a.output, widen=a.widen, drop=a.drop, height=a.height, bands=a.bands, min_size=a.min_size,
                      keep_overlapped=a.keep_overlapped, t_from=a.t_from, t_until=a.t_until, batch=a.batch, ctx=ctx)
    elif a.verb == "link":
        link(a.table, a.output, min_score=a.min_score, margin=a.margin, max_gap=a.max_gap, min_faces=a.min_faces, min_pixels=a.min_pixels,
             labels=a.labels, merged=a.merged)
    elif a.verb == "demo":
        v = video()
        res = demo(v, a.tracking, a.output, height=a.height, t_from=a.t_from, t_until=a.t_until, shift=a.shift, landmark=a.landmark,
                   label=a.label, fps=a.fps, ctx=ctx, **colours(v, a.matrix, a.range))
    elif a.verb == "redact":
        if (a.only is not None or a.keep is not None) and a.label is None:
            ap.error("--only / --keep select by label: they need --label")
        if a.cells < 1 or a.pad < 0:
            ap.error("--cells is at least 1 and --pad at least 0")
        v = video()
        res = redact(v, a.tracking, a.output, height=a.height, t_from=a.t_from, t_until=a.t_until, shift=a.shift, label=a.label, only=a.only,
                     keep=a.keep, pad=a.pad, cells=a.cells, shape=a.shape, mode=a.mode, colour=a.colour, draw=a.draw, fps=a.fps, ctx=ctx,
                     **colours(v, a.matrix, a.range))
    elif a.verb == "faces":
        res = faces(video(), a.tracking, a.landmarks, a.output, per=a.per, tile=a.tile, columns=a.columns, label=a.label, only=a.only,
                    spread=a.spread, min_size=a.min_size, max_dark=a.max_dark, max_bright=a.max_bright, t_from=a.t_from, t_until=a.t_until,
                    index=a.index, quality=a.quality, ctx=ctx)
    elif a.verb == "talk":
        res = talk(video(), a.tracking, a.landmarks, a.output, window=a.window, on=a.on, off=a.off, min_duration=a.min_duration,
                   max_pause=a.max_pause, max_dark=a.max_dark, t_from=a.t_from, t_until=a.t_until, label=a.label, segments=a.segments, ctx=ctx)
    elif a.verb == "tube":
        if len(a.rest) > 2:
            ap.error("tube takes <video> <tracking> [<landmarks>] <output-directory>")
        v = video()
        res = tube(v, a.tracking, a.rest[0] if len(a.rest) == 2 else None, a.rest[-1], size=a.size, region=a.region, scale=a.scale,
                   smooth=a.smooth, label=a.label, only=a.only, segments=a.segments, min_length=a.min_length, t_from=a.t_from,
                   t_until=a.t_until, fmt=a.fmt, index=a.index, fps=a.fps, ctx=ctx, align=a.align,
                   **colours(v, a.out_matrix or a.matrix, a.out_range or a.range))
    elif a.verb == "extract":
        extract(video(), a.landmark_model, a.embedding_model, a.tracking, a.landmarks, a.embeddings, ctx=ctx, num_jitters=a.jitters,
                jitter_seed=a.jitter_seed)
    else:
        cluster(a.embeddings, a.labels, threshold=a.threshold, force=a.force, metric=a.metric, ctx=ctx, do_not_cooccur=a.do_not_cooccur)
    return res


if __name__ == "__main__":
    sys.exit(main())
