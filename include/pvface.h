/*
 * pvface.h -- C ABI of the MI355X-native face hot path (libpvface.so, built from pyannote-video_amd/csrc).
 *
 * This is the drop-in boundary: every entry point replaces one call the reference makes into dlib / scipy /
 * munkres / pyannote.algorithms.  "ref:" lines cite the reference interface (file:line under /root/reference)
 * the function stands in for.  INTEGRATION.md shows the reference-side ctypes binding.
 *
 * Conventions
 *   - every function returns 0 on success, <0 on error; pvf_last_error() gives the thread-local message;
 *     nothing throws or aborts across the boundary;
 *   - handles are opaque uint64_t; the caller owns every host buffer, the library owns device memory;
 *   - TWO HIP streams per context, each with the entry points, the scratch buffers and the lock of its side: the DETECTOR side
 *     (pvf_detect, pvf_detect_batch, pvf_detect_many, pvf_frame_resize: pyramid, FHOG and scoring kernels whose grids fill the chip)
 *     and the rest (trackers, chips, landmarks, embedding, clustering, shot detection: latency-bound chains the host waits on,
 *     on a stream of higher priority).  Calls of one side are serialised by the library (they may come from any thread); a call
 *     of the detector side and a call of the other side run side by side, on the host and on the device -- the streaming engine
 *     detects shot k + 1 in one thread while another tracks and extracts shot k.  Frames are read by both sides; a result the
 *     other side consumes (detections -> tracker starts) passes through the host, which is the ordering between the two streams.
 *     Different contexts (= different GPUs / ranks) run side by side in different threads or processes;
 *   - frames are uint8 RGB, HWC, C-contiguous (ref: pyannote/video/video.py:148-149,400-401);
 *   - there is NO CPU fallback: without a gfx950 device pvf_ctx_create fails.
 */
#ifndef PVFACE_H
#define PVFACE_H
#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef uint64_t pvf_handle;
typedef struct { int32_t left, top, right, bottom; } pvf_rect_i32;   /* dlib.rectangle (inclusive ints) */

/* ---- context ------------------------------------------------------------------------------------- */
const char* pvf_last_error(void);
int32_t pvf_version(void);
int32_t pvf_device_count(int32_t* n);
int32_t pvf_ctx_create(int32_t device, pvf_handle* ctx);
/* same, choosing the priority class of the context's main (non-detector) stream: -1 as low as the detector's stream, 0 / +1 above it */
int32_t pvf_ctx_create_prio(int32_t device, int32_t priority_class, pvf_handle* ctx);
int32_t pvf_ctx_destroy(pvf_handle ctx);
int32_t pvf_sync(pvf_handle ctx);

/* ---- models --------------------------------------------------------------------------------------- */
/* ref: face.py:54  dlib.get_frontal_face_detector()  (path == NULL: detector shipped with the package) */
int32_t pvf_load_detector(pvf_handle ctx, const char* path);
/* ref: face.py:58  dlib.shape_predictor(landmarks); README.md:29-30, scripts/pyannote-face.py:37,451-452 pass dlib's own
 * `shape_predictor_68_face_landmarks.dat` by path: accepted as is (dlib::serialize stream), as is the `.pvfm` container */
int32_t pvf_load_shape_predictor(pvf_handle ctx, const char* path);
/* ref: face.py:62  dlib.face_recognition_model_v1(embedding); `dlib_face_recognition_resnet_model_v1.dat` or `.pvfm` */
int32_t pvf_load_embedder(pvf_handle ctx, const char* path);
/* host only (no GPU needed): one named tensor of a model file exactly as the two loaders above parse it
 * (kind 1 = shape predictor, 2 = embedder; names "sp.*" / "emb.*"); out == NULL returns the size in *nbytes */
int32_t pvf_model_tensor(const char* path, int32_t kind, const char* name, void* out, int64_t cap_bytes, int64_t* nbytes);
/* constant tables of dlib.correlation_tracker's default constructor (ref: tracking.py:250), computed once on the host:
 * mask64[64*64], mask_scale[32], tw64[32*2] (cos,sin 2*pi*k/64), tw32[16*2] */
int32_t pvf_set_tracker_tables(pvf_handle ctx, const double* mask64, const double* mask_scale, const double* tw64,
                               const double* tw32, double alpha_pow_m16, double ln_alpha);

/* ---- frames --------------------------------------------------------------------------------------- */
/* stage a host frame into HBM once; detection, trackers, landmarks and embedding all reuse it
 * (the reference re-reads the host array for every dlib call: tracking.py:203,251,426; pyannote-face.py:296-297) */
int32_t pvf_frame_upload(pvf_handle ctx, const uint8_t* rgb, int32_t h, int32_t w, int64_t row_stride_bytes, pvf_handle* frame);
/* `rgb` may also be a device address (a decoder that delivers into HBM): the frame is copied into a buffer of the library's own, so
 * the source may be overwritten as soon as the call returns */
/* wrap a frame that already lives in HBM (no copy; the caller keeps it alive until pvf_frame_release RETURNS: compute calls queue their
 * kernels without waiting for them, so releasing a wrapped frame waits for the compute stream -- only then may the memory be reused) */
int32_t pvf_frame_wrap_device(pvf_handle ctx, const void* dev_rgb, int32_t h, int32_t w, pvf_handle* frame);
/* Releasing never waits for the GPU: the buffer of a frame the library allocated itself (upload, ingest ring, device resize) goes back
 * to a pool together with an event on the compute stream, and whoever takes it next orders its first write behind that event.
 * The frame calls (upload / wrap / release / ingest) may be made from a second thread (a decoder) while another thread runs the
 * compute entry points of the same context; release a frame only after the calls that use it have returned. */
int32_t pvf_frame_release(pvf_handle ctx, pvf_handle frame);
int32_t pvf_frame_release_many(pvf_handle ctx, const pvf_handle* frames, int32_t n);
/* ref: tracking.py:359-362,410-420 -- the reference drops a shot's frame cache when the shot is done; a streaming run here recycles
 * the buffers of released frames, and this call gives pooled buffers beyond `keep_bytes` back to the allocator (*pooled_bytes,
 * optional: what the pool still holds) */
int32_t pvf_frame_pool_trim(pvf_handle ctx, int64_t keep_bytes, int64_t* pooled_bytes);
/* free / total device memory (hipMemGetInfo): the peak-HBM figure of the streaming runs */
int32_t pvf_mem_info(pvf_handle ctx, int64_t* free_bytes, int64_t* total_bytes);
/* device address of a staged frame (to share it with a second context on the same GPU, e.g. a detector stream) */
int32_t pvf_frame_device_ptr(pvf_handle ctx, pvf_handle frame, const void** dev_rgb);

/* ---- frame ingest ------------------------------------------------------------ */
/* ref: video.py:368-406 (one pipe read + numpy array per frame), :402-403 (cv2.resize), pyannote-face.py:261,287 (two decodes).
 * A ring of `depth` pinned host slots of one frame size; the decoder writes a frame into the slot pvf_ingest_acquire hands out
 * (it returns when that slot's previous upload has left the buffer), pvf_ingest_submit queues ONE asynchronous host-to-HBM copy
 * on the ring's own copy stream and returns a frame handle at once: kernels that read the frame wait for its copy on the device,
 * so uploads overlap the detector.  Release the frame with pvf_frame_release (its buffer is recycled). */
int32_t pvf_ingest_create(pvf_handle ctx, int32_t h, int32_t w, int32_t depth, pvf_handle* ring);
int32_t pvf_ingest_destroy(pvf_handle ctx, pvf_handle ring);
int32_t pvf_ingest_acquire(pvf_handle ctx, pvf_handle ring, int32_t* slot, uint8_t** host_rgb);
int32_t pvf_ingest_submit(pvf_handle ctx, pvf_handle ring, int32_t slot, pvf_handle* frame);
int32_t pvf_ingest_wait(pvf_handle ctx, pvf_handle ring);       /* all queued uploads done (measurement, shutdown) */
/* YUV at ingest ("YUV to RGB"): what a decoder writes -- 8-bit 4:2:0 / 4:2:2 / 4:4:4 -- goes to HBM as it is
 * (1.5 bytes per pixel over PCIe for 4:2:0 where RGB takes 3) and one kernel writes the RGB frame every other call reads.  The
 * reference leaves this to `ffmpeg -pix_fmt rgb24` on the CPU (video.py:332-358).  Integer 16.16 arithmetic, chroma replicated. */
#define PVF_YUV_BT709 1        /* flags: BT.709 matrix (default BT.601) */
#define PVF_YUV_FULL_RANGE 2   /* flags: full range 0..255 (default limited: Y 16..235) */
/* a ring like pvf_ingest_create's whose slots hold one planar frame: Y (h x w), U, V (ceil(w / 2) x ceil(h / 2) each for layout 420;
 * 422 halves the width only, 444 neither), tight, in that order; acquire / submit / wait / destroy work on it unchanged, and submit
 * queues copy + conversion on the ring's copy stream */
int32_t pvf_ingest_create_yuv(pvf_handle ctx, int32_t h, int32_t w, int32_t depth, int32_t layout, int32_t flags, pvf_handle* ring);
/* planes already in HBM (a hardware decoder's surface): pitches in bytes; c_step 1 = planar chroma, 2 = interleaved (NV12: u = uv,
 * v = uv + 1).  Returns when the planes have been read: the surface may be reused at once.  The frame is the library's own (pooled). */
int32_t pvf_frame_from_yuv(pvf_handle ctx, const uint8_t* y, int64_t y_pitch, const uint8_t* u, const uint8_t* v, int64_t c_pitch,
                           int32_t c_step, int32_t h, int32_t w, int32_t layout, int32_t flags, pvf_handle* frame);
/* ref: video.py:180-187,402-403 + tracking.py:389-400  cv2.resize(frame, (w, h)) for detection on down-scaled frames (--min-size):
 * OpenCV's 8-bit INTER_LINEAR on the device; the source frame stays resident for `extract` */
int32_t pvf_frame_resize(pvf_handle ctx, pvf_handle frame, int32_t out_w, int32_t out_h, pvf_handle* out);

/* ---- annotated video out: the `demo` verb (DEMO.md) ------------------------------------------------- */
/* ref: scripts/pyannote-face.py:317-384 (get_make_frame: cv2.resize through video.frame_size, cv2.putText / rectangle / line per face)
 * and :401-413 (moviepy pushes RGB frames to ffmpeg).  One kernel per call resizes the resident frame (the bytes of pvf_frame_resize),
 * draws the frame's primitives in list order (later ones overwrite earlier ones, each clipped to the frame) and converts to planar
 * YUV 4:2:0: Y (out_h x out_w), then U, then V (ceil(out_h / 2) x ceil(out_w / 2) each), tight -- the layout pvf_ingest_create_yuv
 * reads.  Integer arithmetic throughout; DEMO.md states it.  flags: PVF_YUV_BT709 / PVF_YUV_FULL_RANGE.
 * A primitive is eight int32: rectangle outline (a, b, c, d) = (left, top, right, bottom), two pixels wide; line (a, b) - (c, d), one
 * pixel wide; text with (a, b) the bottom-left corner of the first glyph's 5 x 7 box, c and d the offset and length of its bytes in
 * the call's text pool, `scale` the side of a font pixel.  Coordinates are any int32.  colour = r | g << 8 | b << 16.
 * A redaction (REDACT.md) hides the box (a, b, c, d) = (left, top, right, bottom), corners inclusive, or the ellipse inscribed in it:
 * `scale` is the side of a mosaic cell in output pixels, the top byte of `colour` carries PVF_REDACT_* flags.  A covered pixel shows the
 * mean of its cell of the resized source picture (mosaic), a bilinear blend of the neighbouring cells' means (smooth) or `colour`
 * (fill).  `reserved` is the library's: it is overwritten in the device copy of the list, whatever the caller puts there. */
#define PVF_PRIM_RECT 0
#define PVF_PRIM_LINE 1
#define PVF_PRIM_TEXT 2
#define PVF_PRIM_REDACT 3
#define PVF_REDACT_ELLIPSE 1            /* flags bit 0: the ellipse inscribed in the box (otherwise the box) */
#define PVF_REDACT_MOSAIC 0             /* flags bits 1-2: the mode */
#define PVF_REDACT_SMOOTH 2
#define PVF_REDACT_FILL 4
#define PVF_REDACT_MAX_SIDE 16384       /* width and height of a redaction's box */
#define PVF_REDACT_MAX_COORD (1 << 20)  /* |coordinate| of a redaction */
#define PVF_REDACT_MAX_CELL 2048        /* side of a cell: a cell's sum stays below 2^31 */
#define PVF_REDACT_MAX_CELLS 4096       /* cells per redaction */
#define PVF_REDACT_MAX_TABLE (1 << 22)  /* cells of all the redactions of one call */
#define PVF_RENDER_MAX_PRIMS 4096       /* primitives per frame */
#define PVF_RENDER_MAX_RUN 64           /* bytes per text primitive */
#define PVF_RENDER_MAX_TEXT (1 << 20)   /* text bytes per call */
#define PVF_RENDER_MAX_SCALE 64
#define PVF_RENDER_MAX_BATCH 1024       /* frames per pvf_render_batch call */
#define PVF_SHEET_MIN_TILE 48            /* side S of a contact sheet's tiles (FACES.md) */
#define PVF_SHEET_MAX_TILE 600           /* (four weights x 255 + 2 S^2 stays below 2^31) */
#define PVF_SHEET_MAX_SIDE 16384         /* width and height of a sheet */
#define PVF_SHEET_MAX_PIXELS (1 << 26)   /* width x height of a sheet */
#define PVF_SHEET_MAX_TILES 65536        /* tiles of a sheet, and chips of one quality call */
typedef struct { int32_t type, a, b, c, d; uint32_t colour; int32_t scale, reserved; } pvf_prim;
/* n resident frames of one size into `out` (n planar frames, tight; host memory, or device memory with out_on_device = 1); frame i
 * draws prims[start[i] .. start[i + 1]) (start == NULL: nothing is drawn).  Complete when the call returns.  Refused with an error:
 * an unknown or released frame, an output below 2 x 2, a list or a text pool beyond the caps above, a text run outside the pool. */
int32_t pvf_render_batch(pvf_handle ctx, const pvf_handle* frames, int32_t n, int32_t out_w, int32_t out_h, int32_t flags,
                         const int32_t* start, const pvf_prim* prims, const uint8_t* text, int64_t text_bytes,
                         uint8_t* out, int32_t out_on_device);
/* the egress ring, the mirror image of pvf_ingest_*: `depth` pinned host slots of one planar output frame.  pvf_egress_submit renders
 * one frame into the next slot in ring order -- the kernel on the context's main stream, the device-to-host copy behind it on the ring's
 * own copy stream -- and returns at once; pvf_egress_wait blocks until that slot's planes are in host memory and hands them out;
 * pvf_egress_release gives the slot back.  Submit refuses (it does not wait) when the next slot has not been given back.  Rendering
 * frame k + 1 overlaps the copy of frame k and whatever the host does with frame k - 1; wait / release may come from another thread.
 * The source frame may be released as soon as submit has returned (pvf_frame_release: no wait on the GPU). */
int32_t pvf_egress_create(pvf_handle ctx, int32_t out_w, int32_t out_h, int32_t depth, int32_t flags, pvf_handle* ring);
int32_t pvf_egress_destroy(pvf_handle ctx, pvf_handle ring);
int32_t pvf_egress_submit(pvf_handle ctx, pvf_handle ring, pvf_handle frame, const pvf_prim* prims, int32_t n_prims,
                          const uint8_t* text, int64_t text_bytes, int32_t* slot);
int32_t pvf_egress_wait(pvf_handle ctx, pvf_handle ring, int32_t slot, const uint8_t** host_planes);
int32_t pvf_egress_release(pvf_handle ctx, pvf_handle ring, int32_t slot);
/* the drawn picture BEFORE colour conversion, uint8 RGB [out_h][out_w][3] to host memory: tells resize, drawing and conversion apart */
int32_t pvf_debug_render_rgb(pvf_handle ctx, pvf_handle frame, int32_t out_w, int32_t out_h, const pvf_prim* prims, int32_t n_prims,
                             const uint8_t* text, int64_t text_bytes, uint8_t* rgb);
/* the cell means the list's redactions are drawn from, BEFORE composition: the tables of the list's mosaic and smooth redactions,
 * concatenated in list order, a table's cells row-major, 3 bytes (R, G, B) a cell, to host memory.  An inverted box and a fill have no
 * table; a cell wholly outside the frame reads 0, 0, 0.  `capacity` is the size of `means` in bytes: refused when the tables need more. */
int32_t pvf_debug_redact_means(pvf_handle ctx, pvf_handle frame, int32_t out_w, int32_t out_h, const pvf_prim* prims, int32_t n_prims,
                               uint8_t* means, int64_t capacity);

/* ---- S1 detector ---------------------------------------------------------------------------------- */
/* ref: face.py:64-67  for face in self.face_detector_(rgb, 1)  -> dlib.rectangle list, NMS order.
 * scores (optional) receive dlib's detection_confidence (score - threshold). */
int32_t pvf_detect(pvf_handle ctx, pvf_handle frame, int32_t upsample, double adjust_threshold,
                   pvf_rect_i32* out, float* scores, int32_t cap, int32_t* n);
/* same for many frames of identical size in one launch sequence; counts[i] = detections of frame i,
 * written at out[i*cap_per_frame ...] */
int32_t pvf_detect_batch(pvf_handle ctx, const pvf_handle* frames, int32_t n_frames, int32_t upsample,
                         double adjust_threshold, pvf_rect_i32* out, float* scores, int32_t* counts,
                         int32_t cap_per_frame);
/* many frames of one size, processed `batch` at a time with the host post-processing of a batch hidden behind the kernels of
 * the next one; results identical to pvf_detect_batch on each batch (what the pipeline calls once per shot) */
int32_t pvf_detect_many(pvf_handle ctx, const pvf_handle* frames, int32_t n_frames, int32_t batch, int32_t upsample,
                        double adjust_threshold, pvf_rect_i32* out, float* scores, int32_t* counts, int32_t cap);

/* the detector's screening pass (on by default; csrc/screen.hip).  on = 1: every window is first scored on the f16 matrix cores with
 * a proven error bound, and the exact fp32 chain runs only for the windows whose approximate score comes within the bound of the
 * threshold; on = 0: the exact chain is evaluated for every window (score_roll_k).  The rectangles, their order and their scores are
 * the same bits either way -- a call whose list overflows or whose features exceed the bound's assumption is repeated on the dense
 * kernel.  list_cap > 0 sets the (window, filter) pairs a batch may list (default 1 << 20). */
int32_t pvf_detector_screening(pvf_handle ctx, int32_t on, int32_t list_cap);
/* batches screened, (window, filter) pairs listed for exact scoring, calls repeated on the dense kernel -- since the context was created;
 * bounds[0..n_filters) (may be NULL) = the error bound per filter, in score units; pipe_err (may be NULL) = what the context measured
 * on its device before the first screened batch: worst |matrix pipe - exact| / sum of magnitudes over an accumulation of 3200 terms
 * (-1 before that; the bound allows 3200 x 2^-22 = 7.6e-4).  The environment variable PVF_DETECTOR_SCREENING=0 switches screening off
 * for every context the process creates. */
int32_t pvf_detector_screening_stats(pvf_handle ctx, int64_t* batches, int64_t* listed, int64_t* retries, double* bounds, double* pipe_err);

/* the embedder's convolutions on the f16 matrix cores with split operands (on by default; csrc/resnet.hip: conv_tile_k with ConvSplit).  on = 1:
 * every convolution outside the 32-channel stage runs as three f16 products of hi / lo halves (scaled by fixed powers of two) with an
 * fp32 accumulation -- descriptors within the error bound of DESIGN.md section 4, no longer the oracle's chain order; a face whose
 * activations leave the f16 range is embedded again on the exact kernels.  on = 0: the exact fp32 kernels only.  The environment
 * variable PVF_EMBEDDER_SPLIT=0 switches the split off for every context the process creates. */
int32_t pvf_embedder_split(pvf_handle ctx, int32_t on);
/* faces embedded with the split on, faces of those embedded again on the exact kernels, and pipe_err = what the context measured on
 * its device before the first split forward: worst |matrix pipe - exact| / sum of magnitudes over an accumulation of 2304 terms (-1
 * before that; the bound allows 2304 x 2^-22) -- since the context was created */
int32_t pvf_embedder_split_stats(pvf_handle ctx, int64_t* faces, int64_t* reruns, double* pipe_err);

/* ---- S2 correlation tracker ------------------------------------------------------------------------ */
/* ref: tracking.py:250  dlib.correlation_tracker() */
int32_t pvf_tracker_create(pvf_handle ctx, pvf_handle* trk);
/* n trackers at once / n trackers back to the pool: the batched host path creates and kills a few thousand per shot */
int32_t pvf_tracker_create_many(pvf_handle ctx, int32_t n, pvf_handle* trks);
int32_t pvf_tracker_destroy_many(pvf_handle ctx, const pvf_handle* trks, int32_t n);
/* n new trackers that are exact copies (filters, position) of started trackers without a pending deferred update.  The two
 * passes over a shot (tracking.py:184-259 forward, then backward) start one tracker per detection from the same frame and box:
 * the second pass clones instead of recomputing the same filters.  A clone SHARES its source's filters on the device until either
 * side writes them (start_track, a full update, the commit of a deferred update): only then is the 2.4 MB state copied. */
int32_t pvf_tracker_clone_many(pvf_handle ctx, const pvf_handle* src, int32_t n, pvf_handle* dst);
int32_t pvf_tracker_destroy(pvf_handle ctx, pvf_handle trk);
/* ref: tracking.py:251  tracker.start_track(frame, dlib.drectangle(*detection)) ; box = (l,t,r,b) doubles
 * A box with a non-finite coordinate, or of exactly zero width or height, is refused with an error before any GPU work (its chip map
 * would be 0/0); a refused pvf_tracker_start_many leaves EVERY tracker of the call as it was, and the context keeps working.  A box
 * with r < l or b < t (dlib's empty rectangle) is accepted: it gives finite results like dlib's.  Boxes that cross or leave the
 * frame are valid input: pixels outside the frame read as black.  On an all-black chip the response is all zero, the confidence
 * that pvf_tracker_update returns is 0/0 = NaN, and NaN < threshold is false -- the reference keeps such a tracker, see DESIGN.md. */
int32_t pvf_tracker_start(pvf_handle ctx, pvf_handle trk, pvf_handle frame, const double box[4]);
/* ref: tracking.py:203  confidence = tracker.update(frame)   (peak-to-sidelobe ratio) */
int32_t pvf_tracker_update(pvf_handle ctx, pvf_handle trk, pvf_handle frame, double* psr);
/* ref: tracking.py:165,231-237  tracker.get_position() -> drectangle */
int32_t pvf_tracker_position(pvf_handle ctx, pvf_handle trk, double box[4]);
/* batched forms (an addition; the per-object calls above keep working): tracker i runs on frames[i] */
int32_t pvf_tracker_start_many(pvf_handle ctx, const pvf_handle* trks, const pvf_handle* frames,
                               const double* boxes /* n*4 */, int32_t n);
int32_t pvf_tracker_update_many(pvf_handle ctx, const pvf_handle* trks, const pvf_handle* frames, int32_t n,
                                double* psr /* n */, double* boxes_out /* n*4, may be NULL */);
/* update() without the model update: same confidence and position as pvf_tracker_update_many, filters untouched.  The batched
 * host path kills most trackers right after their first update (tracking.py:219-224: a tracker matched to a new detection is
 * dropped), so it defers the filter update and only pays for it -- pvf_tracker_commit_many, with the SAME frames -- for the
 * trackers that live on.  After the commit the tracker state is bit-identical to an immediate update.  A tracker with an
 * uncommitted deferred update refuses further updates. */
int32_t pvf_tracker_update_many_deferred(pvf_handle ctx, const pvf_handle* trks, const pvf_handle* frames, int32_t n,
                                         double* psr, double* boxes_out);
int32_t pvf_tracker_commit_many(pvf_handle ctx, const pvf_handle* trks, const pvf_handle* frames, int32_t n);

/* ---- S3 rectangles + association (host; tiny, order-sensitive) --------------------------------------- */
/* ref: tracking.py:129-134 _match on dlib.drectangle (width = r-l; empty -> area 0), :160-168 overlap matrix */
int32_t pvf_overlap_matrix(const double* a, int32_t na, const double* b, int32_t nb, double ratio, double* out);
/* ref: tracking.py:121,172  Munkres().compute(cost) on the square n x n matrix -> column of each row */
/* _associate (tracking.py:136-182) in one call: gated overlaps, square padding, cost = max - overlap, Munkres, and only the pairs
 * with a positive overlap.  trackers / detections: [n][4] doubles (l,t,r,b); det_of_tracker[t] = detection index or -1. */
int32_t pvf_associate(const double* trackers, int32_t n_trackers, const double* detections, int32_t n_detections,
                      double min_overlap_ratio, int32_t* det_of_tracker);
int32_t pvf_munkres(const double* cost, int32_t n, int32_t* row_to_col);

/* ---- S4 landmarks + embedding ---------------------------------------------------------------------- */
/* ref: face.py:69-70  self.shape_predictor_(rgb, face) -> 68 integer points; face i lives on frames[i].
 * Any int32 box is accepted: zero-area (68 identical points), inverted, off the frame (off-frame pixels read as 0).  The final points
 * SATURATE to the int32 range: floor(x + 0.5) is clamped to [-2^31, 2^31 - 1] as a double, then converted (dlib's behaviour for such
 * boxes is not known: oracle/EXT_REGISTER.md E25).  n = 0 does nothing; refused: n < 0, null pointers with n > 0. */
int32_t pvf_landmarks(pvf_handle ctx, const pvf_handle* frames, const pvf_rect_i32* boxes, int32_t n,
                      int32_t* pts /* n*68*2 */);
/* pvf_landmarks, also returning the float32 shape the last cascade left, in normalised box coordinates (x = left + u * (right - left)):
 * what the integer points are rounded from.  For tests of the order of the kernel's sums. */
int32_t pvf_debug_landmarks_shape(pvf_handle ctx, const pvf_handle* frames, const pvf_rect_i32* boxes, int32_t n,
                                  int32_t* pts /* n*68*2 */, float* shape /* n*68*2 */);
/* ref: face.py:73-76  face_recognition_.compute_face_descriptor(rgb, landmarks) -> 128 floats */
int32_t pvf_embed(pvf_handle ctx, const pvf_handle* frames, const int32_t* pts /* n*68*2 */, int32_t n,
                  float* out /* n*128 */);
/* ref: pyannote-face.py:296-297  landmarks = face.get_landmarks(rgb, face); embedding = face.get_embedding(rgb, landmarks) -- both for a
 * batch of faces in one call (same results as pvf_landmarks followed by pvf_embed) */
int32_t pvf_landmarks_embed(pvf_handle ctx, const pvf_handle* frames, const pvf_rect_i32* boxes, int32_t n,
                            int32_t* pts /* n*68*2 */, float* out /* n*128 */);
/* the network alone on ready-made 150x150x3 chips (host buffer), for testing K7 in isolation */
int32_t pvf_embed_chips(pvf_handle ctx, const uint8_t* chips, int32_t n, float* out /* n*128 */);
/* the aligned chips alone (get_face_chip_details + extract_image_chips), for testing K6 in isolation */
int32_t pvf_face_chips(pvf_handle ctx, const pvf_handle* frames, const int32_t* pts, int32_t n, uint8_t* chips /* n*150*150*3 */);

/* ---- faces: the quality of face chips and the contact sheet (FACES.md; no reference call) -------- */
/* Five int64 per chip (uint8 [150][150][3], what the face chip call returns): S1 = sum of L, S2 = sum of L^2 over
 * the 148 x 148 interior pixels, L the 4-neighbour Laplacian of the luma Y = (77 R + 150 G + 29 B + 128) >> 8; SY = sum of Y,
 * ND = #{Y <= 16}, NB = #{Y >= 239} over all 22 500 pixels.  Integer sums: the result does not depend on the shape of the reduction.
 * The chips come from host memory and go through the device in rounds of 4096.  n = 0 does nothing; refused: n < 0 or beyond
 * PVF_SHEET_MAX_TILES, null pointers with n > 0. */
int32_t pvf_chip_quality(pvf_handle ctx, const uint8_t* chips, int32_t n, int64_t* out /* n*5 */);
/* the same five values for the faces given by frame and 68 landmarks: the chips are made on the device as the embedder's are and
 * reduced there; 40 bytes per face come back.  Needs no embedder: the chip geometry is dlib's mean face shape with a 150-pixel chip
 * and 0.25 padding -- what a dlib embedder file loads -- whichever embedder the context holds. */
int32_t pvf_face_quality(pvf_handle ctx, const pvf_handle* frames, const int32_t* pts /* n*68*2 */, int32_t n, int64_t* out /* n*5 */);
/* The contact sheet: uint8 RGB [H][W][3] to host memory, filled with `background` (r | g << 8 | b << 16); chip i, resampled to S x S
 * (FACES.md "Tile"; S = 150 is the chip itself), with its top-left corner at (xy[2 i], xy[2 i + 1]) -- any int32, clipped to the sheet,
 * a later tile over an earlier one; then the RECT / LINE / TEXT primitives in list order over the tiles, drawn as the renderer above
 * draws them.  n = 0 gives background and primitives.  Refused: S outside PVF_SHEET_MIN_TILE .. PVF_SHEET_MAX_TILE, W or H below 1 or
 * beyond PVF_SHEET_MAX_SIDE, W x H beyond PVF_SHEET_MAX_PIXELS, n beyond PVF_SHEET_MAX_TILES, a background above 0xffffff, a
 * redaction or an unknown primitive, a list or a text pool beyond the PVF_RENDER_MAX_* caps, a text run outside the pool. */
int32_t pvf_chip_sheet(pvf_handle ctx, const uint8_t* chips, int32_t n, const int32_t* xy /* n*2 */, int32_t S, int32_t W, int32_t H,
                       uint32_t background, const pvf_prim* prims, int32_t n_prims, const uint8_t* text, int64_t text_bytes, uint8_t* rgb);
/* the same sheet with the chips made on the device from frames and landmarks (the geometry of the face quality call) */
int32_t pvf_face_sheet(pvf_handle ctx, const pvf_handle* frames, const int32_t* pts /* n*68*2 */, int32_t n, const int32_t* xy, int32_t S,
                       int32_t W, int32_t H, uint32_t background, const pvf_prim* prims, int32_t n_prims, const uint8_t* text,
                       int64_t text_bytes, uint8_t* rgb);

/* ---- talk: how much the mouth of a face chip moved since the face before it (TALK.md; no reference call) -------- */
#define PVF_MOTION_MAX_FACES 32768          /* 32768 x 2 x 46 x 72 B of patches = 217 MB */
/* Eight int32 per face: DM0, DMmin, kM, DC0, DCmin, kC, SM, NZ.  prev[i] is -1 or an index < i of the same call: the face that
 * face i is compared with; several faces may name the same one.  D(dy, dx) is the sum over a window of 40 rows x 64 columns of the chip's
 * luma Y = (77 R + 150 G + 29 B + 128) >> 8 of |Y_i(r, c) - Y_prev(r + dy, c + dx)|, for the 49 shifts in [-3, 3]^2; the mouth window
 * is rows 94 .. 133, the control window rows 52 .. 91, both columns 42 .. 105.  D?0 = D(0, 0), D?min the minimum over the shifts, k? =
 * (dy + 3) * 7 + (dx + 3) of the first minimum in row-major order, but 24 when D(0, 0) is the minimum.  SM = sum of Y over the mouth
 * window, NZ = #{Y <= 16} over both windows.  A face with prev[i] = -1 has -1 in the first six.  Integer sums: nothing depends on the
 * shape of a reduction or on the rounds of 4096 the host chips go through the device in.  n = 0 does nothing; refused: n < 0 or beyond
 * PVF_MOTION_MAX_FACES, null pointers with n > 0, prev[i] < -1, prev[i] >= i. */
int32_t pvf_chip_motion(pvf_handle ctx, const uint8_t* chips, int32_t n, const int32_t* prev, int32_t* out /* n*8 */);
/* the same eight values for faces given by frame and 68 landmarks: the chips are made on the device with the geometry of the face
 * quality call (no embedder needed) and reduced there; 32 bytes per face come back. */
int32_t pvf_face_motion(pvf_handle ctx, const pvf_handle* frames, const int32_t* pts /* n*68*2 */, int32_t n, const int32_t* prev, int32_t* out /* n*8 */);

/* ---- tube: square windows of resident frames as S x S pictures (TUBE.md; no reference call) -------------------- */
#define PVF_CROP_MIN_SIZE 1              /* side S of a picture */
#define PVF_CROP_MAX_SIZE 1024           /* (1024 S^2 x 255 < 2^38: the enlarging sums are 64-bit) */
#define PVF_CROP_MIN_SIDE 16             /* side L of a window in sixteenths of a source pixel: one pixel */
#define PVF_CROP_MAX_SIDE (1 << 18)      /* 16384 pixels: a row's weighted sum stays below L x 255 < 2^26, the picture's below L^2 x 255 < 2^44 */
#define PVF_CROP_MAX_COORD (1 << 30)     /* |X0|, |Y0| in sixteenths: X0 >> 4 plus a window's pixels stays far inside int32 */
#define PVF_CROP_MAX_CROPS 65536         /* crops of one call */
#define PVF_CROP_YUV420 4                /* flags: planar YUV 4:2:0 pictures (default: interleaved RGB); with PVF_YUV_BT709 / PVF_YUV_FULL_RANGE */
/* n pictures of S x S pixels, tight and in call order: picture i is the window windows[3 i .. 3 i + 2] = (X0, Y0, L) of frame frames[i],
 * left edge, top edge and side of a square in sixteenths of a source pixel, any sign and position; outside the frame reads black.
 * L >= 16 S: the exact area average, (sum wy wx byte + L^2 // 2) // L^2; L < 16 S: bilinear at the sample centres,
 * (sum of four weights x bytes + 512 S^2) // (1024 S^2); TUBE.md states both, integer arithmetic throughout.  A picture is RGB [S][S][3]
 * or, with PVF_CROP_YUV420, Y [S][S] then U and V [ceil(S / 2)]^2 of the RGB picture, converted as pvf_render_batch converts (the two
 * colour flags mean nothing without it).  out: host memory, or with out_on_device device memory; the call is complete when it returns.
 * Crops go through the device in rounds (32 MiB of pictures, or the crops the environment variable PVF_CROP_ROUND names, read at the
 * call), a round's copy to the host running under the next round's kernel; nothing depends on the rounds.  n = 0 does nothing.
 * Refused before any work: n < 0 or beyond PVF_CROP_MAX_CROPS, null pointers with n > 0, S or L outside their caps, X0 or Y0 beyond
 * PVF_CROP_MAX_COORD, unknown flag bits, an unknown or released frame. */
int32_t pvf_frame_crops(pvf_handle ctx, const pvf_handle* frames, const int32_t* windows /* n*3 */, int32_t n, int32_t S, int32_t flags,
                        uint8_t* out, int32_t out_on_device);

/* ---- tube --align: oriented windows (TUBE.md "Oriented window"; no reference call) ------------------------------- */
#define PVF_WARP_MAX_K 16                /* sub-samples per output pixel and axis: K^2 x 65536 x 255.5 < 2^32, a pixel's sum is 32-bit */
#define PVF_WARP_MAX_STEP (1 << 20)      /* |BX|, |BY| in 1/65536 pixel: a sub-step of 16 pixels, from where aliasing is accepted */
/* n pictures of S x S pixels as pvf_frame_crops returns them (layouts, flags, rounds, where out lies, n = 0), through windows that
 * need not be axis-aligned: picture i is the window windows[5 i .. 5 i + 4] = (CX, CY, BX, BY, K) of frame frames[i].  (CX, CY): the
 * centre in sixteenths of a source pixel; (BX, BY): the step between sub-samples along an output row in 1/65536 pixel, (-BY, BX) down
 * a column; K x K sub-samples, bilinear with 8-bit fractions, make an output pixel:
 * (sum of their four weighted taps + 32768 K^2) // (65536 K^2); outside the frame reads black.  TUBE.md states the positions; integer
 * arithmetic throughout.  (0, 0) is a valid step.  Refused before any work for pvf_frame_crops' reasons (S, n, |CX|, |CY| <=
 * PVF_CROP_MAX_COORD, flags, pointers, frames) and for K outside 1 .. PVF_WARP_MAX_K or |BX|, |BY| beyond PVF_WARP_MAX_STEP. */
int32_t pvf_frame_warps(pvf_handle ctx, const pvf_handle* frames, const int32_t* windows /* n*5 */, int32_t n, int32_t S, int32_t flags,
                        uint8_t* out, int32_t out_on_device);

/* ---- the storyboard verb (STORYBOARD.md): whole frames as small pictures, and the sheet of them -----------------------------------*/
#define PVF_THUMB_MAX_SIDE 1024          /* tw and th of a thumbnail */
#define PVF_THUMB_MAX_FRAMES 65536       /* frames of one pvf_frame_thumbs call */
/* n RGB pictures [th][tw][3], tight and in call order: picture i is the whole of frame frames[i], all frames of one size (h, w), as the
 * exact area average.  With x in units of 1 / tw source pixel, source column j is [j tw, (j + 1) tw), output column X is [X w, (X + 1) w)
 * and wx(X, j) the length they share (sum over j: w); rows the same with th, h and wy (sum: h);
 *   pixel(Y, X, c) = (sum_i sum_j wy(Y, i) wx(X, j) byte(i, j, c) + (w h) // 2) // (w h)
 * in 64-bit integers.  One rule for every ratio on either axis: tw = w, th = h is the frame byte for byte, an integer reduction the mean
 * rounded half up, an integer enlargement replication.  out: host memory, or device memory with out_on_device = 1; the call is complete
 * when it returns.  Pictures go through the device in rounds (32 MiB of them, or the pictures the environment variable PVF_THUMB_ROUND
 * names, read at the call), a round's copy to the host running under the next round's kernel; nothing depends on the rounds.  n = 0
 * does nothing.  Refused before any work: n < 0 or beyond PVF_THUMB_MAX_FRAMES, null pointers with n > 0, tw or th outside
 * 1 .. PVF_THUMB_MAX_SIDE, flags other than 0, an unknown or released frame, frames of different sizes. */
int32_t pvf_frame_thumbs(pvf_handle ctx, const pvf_handle* frames, int32_t n, int32_t tw, int32_t th, int32_t flags,
                         uint8_t* out /* n*th*tw*3 */, int32_t out_on_device);
/* pvf_chip_sheet with rectangular tiles that are copied, not resampled: the sheet [H][W][3] (host) is filled with the background
 * (r | g << 8 | b << 16); thumbnail i of `thumbs` (host, [n][th][tw][3]) sits with its top-left corner at (xy[2 i], xy[2 i + 1]) -- any
 * int32, clipped to the sheet, the tile of the highest index that covers a pixel wins, whatever the rounds (PVF_THUMB_ROUND tiles, or
 * 32 MiB of them); then the RECT / LINE / TEXT primitives in list order over the tiles, drawn as the renderer draws them.  n = 0 gives
 * background and primitives.  Refused: pvf_chip_sheet's reasons (PVF_SHEET_MAX_*, PVF_RENDER_MAX_*, a redaction or an unknown
 * primitive, a text run outside the pool, null pointers), and tw or th outside 1 .. PVF_THUMB_MAX_SIDE. */
int32_t pvf_thumb_sheet(pvf_handle ctx, const uint8_t* thumbs /* n*th*tw*3 */, int32_t n, const int32_t* xy /* n*2 */, int32_t tw, int32_t th,
                        int32_t W, int32_t H, uint32_t background, const pvf_prim* prims, int32_t n_prims, const uint8_t* text,
                        int64_t text_bytes, uint8_t* rgb /* H*W*3 */);

/* ---- num_jitters (JITTER.md) ------------------------------------------------------------------------
 * dlib: compute_face_descriptor(img, shape, num_jitters) -- the descriptor is the fp32 mean of the network's outputs on J = num_jitters
 * perturbed copies of the aligned chip (shift, zoom, rotation, mirror).  The transform of jitter j is a function of (seed, j) alone,
 * the same for every face of every call.  J of 0 or 1: the plain descriptor, through the plain entry.  J < 0 and J > 4096 are refused.
 * Faces go through in rounds of max(1, 4096 / J); the environment variable PVF_JITTER_CHUNK (chips per round, read at the call) lowers
 * that without changing a bit of the result. */
#define PVF_JITTER_ROW 17
/* ref: compute_face_descriptor(img, shape, num_jitters).  Host only (no context, no device): the J transforms.  Row j, 17 doubles:
 *   [0..3] l t r b   the chip_details rectangle on the 150 x 150 chip      [4] cs = cos(angle)   [5] sn = sin(angle)
 *   [6]    flip      1.0: output column c takes extracted column 149 - c
 *   [7..10] m[4], [11..12] b[2]   the sampling affine: px = m0 c + m1 r + b0, py = m2 c + m3 r + b1, relative to (bx0, by0)
 *   [13..16] bx0 by0 sw sh        the clipped, grown bounding box the black-outside test is relative to */
int32_t pvf_jitter_plan(int32_t J, uint64_t seed, double* out /* J*17 */);
/* ref: compute_face_descriptor(img, shape, num_jitters) -- dlib's jitter_image alone: host chips [n][150][150][3] in, the n*J jittered
 * chips [n][J][150][150][3] out (jitter_k), for testing the step in isolation; J >= 1 */
int32_t pvf_debug_jitter_chips(pvf_handle ctx, const uint8_t* chips, int32_t n, int32_t J, uint64_t seed, uint8_t* out);
/* ref: compute_face_descriptor(img, shape, num_jitters) -- a measurement switch: the same sampling by transform_k launched over n*J
 * jobs on the chips in HBM (profiling family "jitter_xf"; jitter_k's is "jitter").  transform_k has no mirror: jitters with flip = 1
 * come out unmirrored, everything else is pvf_debug_jitter_chips' output.  out may be NULL: the kernels run, nothing is copied out. */
int32_t pvf_debug_jitter_chips_transform(pvf_handle ctx, const uint8_t* chips, int32_t n, int32_t J, uint64_t seed, uint8_t* out);
/* ref: compute_face_descriptor(img, shape, num_jitters) -- pvf_embed with jitters; J <= 1 returns pvf_embed's bits */
int32_t pvf_embed_jitter(pvf_handle ctx, const pvf_handle* frames, const int32_t* pts /* n*68*2 */, int32_t n, int32_t J, uint64_t seed,
                         float* out /* n*128 */);
/* ref: compute_face_descriptor(img, shape, num_jitters) -- pvf_landmarks_embed with jitters (same results as pvf_landmarks followed by
 * pvf_embed_jitter); J <= 1 returns pvf_landmarks_embed's bits */
int32_t pvf_landmarks_embed_jitter(pvf_handle ctx, const pvf_handle* frames, const pvf_rect_i32* boxes, int32_t n, int32_t J,
                                   uint64_t seed, int32_t* pts /* n*68*2 */, float* out /* n*128 */);
/* ref: compute_face_descriptor(img, shape, num_jitters) -- pvf_embed_chips with jitters (host chips); J <= 1 returns its bits */
int32_t pvf_embed_chips_jitter(pvf_handle ctx, const uint8_t* chips, int32_t n, int32_t J, uint64_t seed, float* out /* n*128 */);

/* ---- S5 clustering --------------------------------------------------------------------------------- */
/* ref: clustering.py:100-112  -squareform(pdist(X,'euclidean')) reduced to the T x T matrix of block means;
 * X float64 [N][dim], rows grouped by track, row_start[T+1]; D float64 [T][T] (positive distances).
 * Like the reference (clustering.py:104-112: itertools.combinations(range(n_clusters), 2), matrix[i, j] = matrix[j, i]) only the
 * track pairs i < j are computed; D[j][i] is a copy of D[i][j], the diagonal is zero.
 * row_start, in every entry of this section: checked on the host before any device work (csrc/group_blocks.h, the check of the
 * identification entries below) -- it starts at 0, is non-decreasing, has NO EMPTY TRACK and ends at N; otherwise the call returns an
 * error and writes nothing.  The entries that take a matrix instead of rows (pvf_cluster_dist, pvf_cluster_upper and their _cooccur
 * siblings) have no N: row_start gives them the track sizes, and the same rules hold with N = row_start[T].  The float32 entries read
 * order[k] for every k < N: `order`, when given, holds N entries. */
int32_t pvf_pair_mean_dist(pvf_handle ctx, const double* X, int32_t N, int32_t dim, const int32_t* row_start,
                           int32_t T, double* D);
/* same with the pair distance chosen: metric 0 = Euclidean (the reference, clustering.py:101), 1 = cosine distance 1 - a.b / (|a| |b|)
 * (BASELINE.json north_star's wording; 128-D rows).  pvf_cluster_dist agglomerates either matrix. */
int32_t pvf_pair_mean_dist_metric(pvf_handle ctx, const double* X, int32_t N, int32_t dim, const int32_t* row_start,
                                  int32_t T, int32_t metric, double* D);
/* ---- the host state machine of one shot, array in / array out (csrc/shotgraph.hip) ----------------------------------------------
 * ref: pyannote/video/tracking.py:184-259 (_track: one pass over a shot), :261-357 (_fix, _fill_gaps, components, (min_t, max_t) sort);
 *      scripts/pyannote-face.py:125-127,142-145,262-266 (the track file's numbers).  No device work: pure host code, callable without a
 *      context.  A pass ("lane") is resumable: the trackers' starts and first updates are issued ahead in bulk (the plan, fed by the
 *      caller), and the lane only comes back for trackers that outlive their first update.
 * direction / node kinds: 1 forward, 2 detection, 3 backward (the reference's status order). */
int32_t pvf_lane_create(int32_t n_frames, const int32_t* det_counts /* per shot frame */, const double* det_boxes /* [sum][4], frame after frame */,
                        int32_t direction, double min_confidence, double min_overlap_ratio, int32_t deferring, pvf_handle* lane);
int32_t pvf_lane_destroy(pvf_handle lane);
/* plan of the PROCESSING frames [p0, p0 + n_p) (backward pass: frame n - 1 - p): has_update[n_p]; for the detections of those frames in
 * processing order the tracker handle and its first update's confidence + position (ignored where has_update is 0) */
int32_t pvf_lane_feed_plan(pvf_handle lane, int32_t p0, int32_t n_p, const uint8_t* has_update, const uint64_t* handles, const double* psr,
                           const double* pos);
/* run until the pass ends or needs the caller: *request 0 done, 1 update (reply_psr / reply_pos [n][4] with the NEXT call), 2 commit,
 * 3 plan wanted from processing frame *plan_from; req_handles / req_frames (shot frame indices) name the trackers of requests 1 and 2 */
int32_t pvf_lane_advance(pvf_handle lane, const double* reply_psr, const double* reply_pos, int32_t n_reply, int32_t* request,
                         uint64_t* req_handles, int32_t* req_frames, int32_t cap, int32_t* n_req, int32_t* plan_from);
int32_t pvf_lane_take_dead(pvf_handle lane, uint64_t* out, int32_t cap, int32_t* n);      /* killed trackers, to be released by the caller */
int32_t pvf_lane_edges(pvf_handle lane, int32_t* n_edges, int32_t* u_frame_kind, double* u_box, int32_t* v_frame_kind, double* v_box,
                       double* conf, int32_t cap);                                         /* add_edge calls of the pass, in order */
/* tracks of the shot from its two finished passes: rows [cap][6] = (frame, l, t, r, b, status code: forwards | detections << 8 |
 * backwards << 16 | error << 24); track k = rows track_start[k] .. track_start[k + 1]; counts beyond the caps: nothing written */
int32_t pvf_shot_tracks(pvf_handle lane_forward, pvf_handle lane_backward, const double* times, int32_t n_frames, double max_gap,
                        int32_t* rows, int32_t cap, int32_t* n_rows, int32_t* track_start, int32_t track_cap, int32_t* n_tracks);
/* file_box = float64(float32(round(box / detection size, 3))), pixel_box = int(file_box * frame size): what `track` writes and `extract` reads */
int32_t pvf_track_rows(const int32_t* boxes, int64_t n, int32_t det_width, int32_t det_height, int32_t width, int32_t height,
                       double* file_box, int32_t* pixel_box);
int32_t pvf_round_decimals(const double* in, int64_t n, int32_t decimals, double* out);    /* Python's round(float, decimals), array form */

/* ref: clustering.py:116-119,138-148  FaceClustering(threshold)(starting_point, features): average-linkage HAC from the
 * track partition, stop when the closest pair's mean distance exceeds `threshold`;
 * labels[t] = smallest track index of t's cluster; merge_log optional [(T-1)*4] = (a, b, dist, new_size) */
/* The two halves of pvf_cluster_tracks for several GPUs sharing one global clustering (dist.py).
 * pvf_pair_mean_dist_rows: the COMPLETE rows [track0, track1) of the T x T matrix of pvf_pair_mean_dist (D: T x T, row-major; other
 *   rows are left untouched) -- entries j > i computed, entries j < i the mirror of D[j][i] (clustering.py:111-112), diagonal 0; what
 *   this entry has returned since round 2 (round 4 silently left the part below the diagonal zero: restored in round 5).  COST: the
 *   mirrored part of row i is column i of the rows above it, so the rows [0, track1) are computed, not only [track0, track1) -- for the
 *   last share of a split that is the whole matrix, O(T^2): a job that splits the work calls pvf_pair_upper_rows (dist.py does).
 * pvf_pair_upper_rows: only the UPPER-TRIANGLE entries D[i][j], i < j, of those rows (entries j <= i written as zeros): the share a
 *   rank contributes when the ranks split the pairs by triangle area -- nothing is computed twice.
 * Then the agglomeration of a complete D (pvf_cluster_dist) or of the assembled upper triangle (pvf_cluster_upper mirrors it first).
 * Every entry is produced by the same chain of additions as in the single call, so row ranges computed by different ranks stitch
 * into the single call's matrix bit for bit. */
int32_t pvf_pair_mean_dist_rows(pvf_handle ctx, const double* X, int32_t N, int32_t dim, const int32_t* row_start, int32_t T,
                                int32_t track0, int32_t track1, double* D);
int32_t pvf_pair_upper_rows(pvf_handle ctx, const double* X, int32_t N, int32_t dim, const int32_t* row_start, int32_t T,
                            int32_t track0, int32_t track1, double* D);
int32_t pvf_cluster_dist(pvf_handle ctx, const double* D, const int32_t* row_start, int32_t T, double threshold,
                         int32_t* labels, double* merge_log, int32_t* n_merges);
/* U: T x T with the entries i < j set (anything below the diagonal is ignored), in host (on_device = 0) or device memory */
int32_t pvf_cluster_upper(pvf_handle ctx, const double* U, int32_t on_device, const int32_t* row_start, int32_t T, double threshold,
                          int32_t* labels, double* merge_log, int32_t* n_merges);
int32_t pvf_cluster_tracks(pvf_handle ctx, const double* X, int32_t N, int32_t dim, const int32_t* row_start,
                           int32_t T, double threshold, int32_t* labels, double* merge_log, int32_t* n_merges);
/* ref: clustering.py:142-143  `# constraint = DoNotCooccur()` / `constraint = None`: the constraint the reference names and leaves
 * switched off, here as siblings of the four agglomerating entries.  [EXT pyannote.algorithms, absent; PARITY UNPINNED]
 *   extent    T x 2 float64, (start, end) of each track in seconds (first and last timestamp of its rows, clustering.py:76-77).  NULL is
 *             refused: the entries without a constraint stay for that.  A value that is not finite, or end < start, is refused.
 *             Tracks i != j CO-OCCUR iff  min(end_i, end_j) - max(start_i, start_j) > 1e-6  (float64, this form: a non-empty
 *             intersection by pyannote.core's Segment rule).  A pair of clusters holding a co-occurring pair of tracks is never
 *             merged and never stops the loop: the agglomeration ends when no mergeable pair is left or the closest mergeable pair
 *             lies above `threshold` -- with threshold = +inf that may leave more than one cluster.  Without co-occurring tracks
 *             the result is that of the entry without a constraint, bit for bit.
 *   n_blocked output: the co-occurring pairs i < j.
 *   flags     bit 0: A TEST SWITCH -- run the launch-per-merge agglomeration (otherwise used above 10 200 tracks only) whatever T, so
 *             that path can be checked at small T; same result, slower.  Other bits must be zero. */
int32_t pvf_cluster_dist_cooccur(pvf_handle ctx, const double* D, const int32_t* row_start, int32_t T, double threshold,
                                 int32_t* labels, double* merge_log, int32_t* n_merges, const double* extent, int32_t* n_blocked,
                                 int32_t flags);
/* ref: clustering.py:142-143 */
int32_t pvf_cluster_upper_cooccur(pvf_handle ctx, const double* U, int32_t on_device, const int32_t* row_start, int32_t T,
                                  double threshold, int32_t* labels, double* merge_log, int32_t* n_merges, const double* extent,
                                  int32_t* n_blocked, int32_t flags);
/* ref: clustering.py:142-143 */
int32_t pvf_cluster_tracks_cooccur(pvf_handle ctx, const double* X, int32_t N, int32_t dim, const int32_t* row_start, int32_t T,
                                   double threshold, int32_t* labels, double* merge_log, int32_t* n_merges, const double* extent,
                                   int32_t* n_blocked, int32_t flags);
/* The in-memory path (no embedding.txt in between): the float32 descriptors as pvf_embed returned them -- `emb` is a host or a device
 * address (emb_on_device), n_src rows of 128 floats row_stride_bytes apart.  Row k of the clustering's table is
 * np.round(float64(emb[order[k]]), decimals) -- what the reference reads back from the '%.5f' text (pyannote-face.py:307-311,
 * clustering.py:70-75; decimals < 0: no rounding; order NULL: rows as they are) -- gathered and rounded ON THE DEVICE: one upload of
 * 4 bytes per value (none when the rows are in HBM already, e.g. the gathered rows of a multi-GPU run) instead of host passes over an
 * 8-byte table.  128-D rows.  pvf_pair_upper_rows_f32 writes the (track1 - track0) x T values of its rows compactly into rows_out
 * (host or device memory): the share one rank contributes to the all-gather of D. */
int32_t pvf_cluster_tracks_f32(pvf_handle ctx, const float* emb, int64_t row_stride_bytes, int32_t n_src, int32_t emb_on_device,
                               const int32_t* order, int32_t N, int32_t decimals, const int32_t* row_start, int32_t T, int32_t metric,
                               double threshold, int32_t* labels, double* merge_log, int32_t* n_merges);
/* ref: clustering.py:142-143  pvf_cluster_tracks_f32 with the do-not-cooccur constraint (extent, n_blocked, flags: see above) */
int32_t pvf_cluster_tracks_f32_cooccur(pvf_handle ctx, const float* emb, int64_t row_stride_bytes, int32_t n_src, int32_t emb_on_device,
                                       const int32_t* order, int32_t N, int32_t decimals, const int32_t* row_start, int32_t T,
                                       int32_t metric, double threshold, int32_t* labels, double* merge_log, int32_t* n_merges,
                                       const double* extent, int32_t* n_blocked, int32_t flags);
int32_t pvf_pair_upper_rows_f32(pvf_handle ctx, const float* emb, int64_t row_stride_bytes, int32_t n_src, int32_t emb_on_device,
                                const int32_t* order, int32_t N, int32_t decimals, const int32_t* row_start, int32_t T,
                                int32_t track0, int32_t track1, double* rows_out, int32_t out_on_device);

/* ---- identification against a gallery ----------------------------------------------------------------------------------------------
 * WHO a face is: query rows X float64 [N][dim] in T groups (row_start[T+1]; a group is a track or a cluster), gallery rows G float64
 * [M][dim] in K identities (gal_start[K+1]: the enrolled descriptors of each known person).  There is NO REFERENCE CALL: naming a 128-D
 * descriptor by its distance to known faces is the use the embedder was trained for ("below 0.6 is the same person"), the reference
 * offers none.  The measure is the one pvf_cluster_tracks merges by: a group belongs to an identity when the MEAN PAIRWISE DISTANCE
 * between its rows and the identity's rows is at most `threshold` -- one more average-linkage step against fixed, named clusters.
 * `metric` and `threshold` mean what they mean in pvf_cluster_tracks / pvf_pair_mean_dist_metric (0 Euclidean, 1 cosine distance,
 * 0 where a norm is 0; `<=`; the default of the callers is 0.6).
 *   D[t][k]  = mean over the rows i of group t and the rows j of identity k of dist(x_i, g_j), float64, T x K row-major, computed on the
 *              f64 matrix cores by the rectangular form of K10; neither N x M nor N x K is materialised.  Defined up to rounding
 *              (rtol 1e-12 Euclidean, 1e-10 cosine), not bit for bit: the additions that form an entry depend on where the rows of the
 *              group and of the identity fall in their 16-row blocks.  The same call returns the same bits.  Euclidean pairs with
 *              d^2 < 1e-3 (|x_i|^2 + |g_j|^2) are summed from their differences (identical rows: exactly 0); the others take
 *              |x|^2 + |g|^2 - 2 x.g, whose relative error in d, C 2^-53 (|x|^2 + |g|^2) / d^2 with C <= 4.5 measured, is at most 5e-13
 *              there, at any scale of the rows.  pvf_pair_mean_dist* (K10) computes the pairs of 128-D rows the same way.
 *   decision per group t: an entry is TAKEN when it is below +inf (NaN and +inf entries are never taken).  best = the index of the first
 *              minimum of row t among the taken entries (the lowest k wins on equal values); second = the first minimum over k != best.
 *              A row with nothing to take gives (-1, +inf); with K = 1 the second is (-1, +inf).  Then best = -1 unless
 *              best_dist <= threshold (NaN is refused as a threshold); best_dist keeps the measured value either way.
 * Checked on the host before any device work: T, K >= 1; dim == 128; row_start and gal_start start at 0, are non-decreasing, have no
 * empty group and end at N and M; sizes that 32-bit offsets cannot address (2^30 rows, an identity of 2^20 rows) are refused.
 * pvf_identify_dist: the decision alone, on a host matrix.  pvf_identify: both, D stays in HBM in between; D (T x K, host) may be NULL. */
int32_t pvf_gallery_mean_dist(pvf_handle ctx, const double* X, int32_t N, const int32_t* row_start, int32_t T, const double* G, int32_t M,
                              const int32_t* gal_start, int32_t K, int32_t dim, int32_t metric, double* D /* T x K, host */);
int32_t pvf_identify_dist(pvf_handle ctx, const double* D, int32_t T, int32_t K, double threshold, int32_t* best, double* best_dist,
                          int32_t* second, double* second_dist);
int32_t pvf_identify(pvf_handle ctx, const double* X, int32_t N, const int32_t* row_start, int32_t T, const double* G, int32_t M,
                     const int32_t* gal_start, int32_t K, int32_t dim, int32_t metric, double threshold, int32_t* best, double* best_dist,
                     int32_t* second, double* second_dist, double* D /* T x K host, or NULL */);

/* ---- search: the exact k nearest rows of a table (SEARCH.md) ------------------------------------------------------------------------
 * WHERE ELSE a face appears: for every query row of Qrows float64 [Q][dim] the k nearest rows of X float64 [N][dim], the table: the rows
 * of one or many embedding files.  There is NO REFERENCE CALL.  Euclidean only, and EXACT: the rules are stated in integers.
 *   quantisation  q(v) = rint(v * 100000.0), the product in float64, ties to even: the integer a 5-decimal value stands for.  A table or
 *              a query holding a value that is not finite, or with |q| > 2^20 (|v| above about 10.48), is REFUSED as a whole; the message
 *              names the row and column of the first such value in row-major order.  Nothing is clamped, and no result is computed.
 *   distance   d2(a, b) = sum over c of (q(a_c) - q(b_c))^2, an exact integer in [0, 2^49].  sqrt(d2) / 1e5 is what people read; it is
 *              never compared.
 *   hits of a query: the rows i that are not excluded and, with a cut, have d2 <= max_d2 (-1: no cut), ordered by (d2, i) ascending; the
 *              first k are kept.  The order is total, so the result is unique: the same bits whatever the chunking and the device.
 *   exclusion  with row_group int32 [N] and query_group int32 [Q] (both, or both NULL): row i is skipped for query q when
 *              row_group[i] == query_group[q] >= 0 -- a query taken from a track of the table does not find its own track.
 *   outputs    count[q] = min(k, number of hits); idx int32 [Q][k] and d2 int64 [Q][k], both -1 past count[q].
 * Checked on the host before any device work: dim == 128; Q, N >= 1; 1 <= k <= 1024 (a k above N is legal: the tail is -1);
 * N <= 2^30; max_d2 >= -1; the two group arrays together.  The table is streamed through HBM in chunks of rows (PVF_SEARCH_CHUNK, read
 * at every call, sets the rows per chunk: the test switch); Q x N is never written anywhere: device memory is O(chunk + Q k ranges).
 * pvf_search_plan (host only): how a call of these sizes is cut -- out = {rows per chunk, chunks, column ranges per chunk, 16-row blocks
 * per range, entries of a query's pending region, bytes of the selection arena}. */
int32_t pvf_search(pvf_handle ctx, const double* Qrows, int32_t Q, const double* X, int64_t N, int32_t dim, int32_t k,
                   int64_t max_d2, const int32_t* query_group, const int32_t* row_group,
                   int32_t* idx /* Q x k */, int64_t* d2 /* Q x k */, int32_t* count /* Q */);
int32_t pvf_search_plan(int32_t Q, int64_t N, int32_t k, int64_t out[6]);

/* ---- cast: rank-order clustering on an exact k-NN graph (CAST.md) ---------------------------------------------------------------------
 * WHO the people of many films are: the N rows of X float64 [N][dim] are grouped into persons.  There is NO REFERENCE CALL.  Every rule is
 * stated in integers (CAST.md), so labels are a pure function of the inputs.
 *   nodes      rows are quantised and refused as pvf_search does (the message names X[r][c]).  group int32 [N], or NULL: negative = none,
 *              else a value in 0 .. N-1; rows of equal group start joined and never appear in each other's lists.
 *   lists      L_a = the hits of pvf_search for row a against the whole table by (d2, row), the first k, under the cut max_d2 (-1: none),
 *              without a itself and without the rows of a's group.  c_a = len(L_a); O_a(b) = 1-based position of b in L_a.
 *   links      for b in L_a: miss(x -> y) = #{z in L_x[0:p] : z != y, z not in L_y}, p = O_x(y) or c_x when y is not in L_x;
 *              m = miss(a -> b) + miss(b -> a); r = the smaller of the ranks O_a(b), O_b(a) that exist; linked when m * den <= num * r.
 *   labels     connected components of links + group edges; labels[a] = the smallest row of a's component; n_components (may be NULL).
 * Checked on the host before any device work: dim == 128; 1 <= N <= 2^24; 1 <= k <= 256; max_d2 >= -1; 0 <= num <= 2^20; 1 <= den <= 2^20;
 * groups negative or below N.  The table is uploaded once and stays on the device; the lists never leave it.  PVF_CAST_QBLOCK (read at
 * every call; the test switch) sets the query rows per batch, PVF_SEARCH_CHUNK the table rows per chunk.
 * pvf_debug_cast_lists: the lists -- idx int32 [N][k], d2 int64 [N][k], both -1 past count [N].
 * pvf_debug_cast_links: per (a, slot) m and r (int32 [N][k], -1 past the count) and linked (uint8 [N][k], 0 past the count).
 * pvf_cast_plan (host only): out = {query rows per batch, batches, table rows per chunk, chunks, column ranges per chunk, device bytes}. */
int32_t pvf_cast(pvf_handle ctx, const double* X, int64_t N, int32_t dim, int32_t k, int64_t max_d2, int64_t num, int64_t den,
                 const int32_t* group /* N, or NULL */, int32_t* labels /* N */, int32_t* n_components /* or NULL */);
int32_t pvf_debug_cast_lists(pvf_handle ctx, const double* X, int64_t N, int32_t dim, int32_t k, int64_t max_d2, const int32_t* group,
                             int32_t* idx, int64_t* d2, int32_t* count);
int32_t pvf_debug_cast_links(pvf_handle ctx, const double* X, int64_t N, int32_t dim, int32_t k, int64_t max_d2, int64_t num, int64_t den,
                             const int32_t* group, int32_t* m, int32_t* r, uint8_t* linked);
int32_t pvf_cast_plan(int64_t N, int32_t k, int64_t out[6]);

/* ---- footage shared between films (REPEAT.md; no reference call) -----------------------------------------------------------------
 * A print of a frame is four uint64: H, V, SY | RANGE << 32 and a word for the caller.  With G the 9 x 9 thumbnail of the whole frame
 * (pvf_frame_thumbs' exact area average, tw = th = 9; a side below 9 replicates) and Y[r][c] = (77 R + 150 G + 29 B + 128) >> 8 of it:
 * bit 8 r + c of H is Y[r][c] < Y[r][c + 1], of V is Y[r][c] < Y[r + 1][c] (r, c in 0 .. 7), SY is the sum of the 81 Y, RANGE their
 * max - min.  pvf_frame_prints writes the prints of n resident frames, of any sizes, in call order: out uint64 [n][4] in host memory, or
 * in device memory with out_on_device = 1; the fourth word is written as 0.  n = 0 does nothing.  Refused before any work: n < 0 or
 * beyond PVF_PRINT_MAX_ROWS, null pointers with n > 0, an unknown or released frame.
 *
 * pvf_print_runs: rows a of A and b of B (uint64 [N][2]: H, V) match when usable_a[a] and usable_b[b] are non-zero and
 * popcount(Ha ^ Hb) + popcount(Va ^ Vb) <= tau.  A run (i, j, len) is a maximal sequence of matching pairs (i + t, j + t), t < len.
 * Every run with len >= min_len is reported, ordered by (j - i, i).  B == NULL is self mode: B is A (usable_b and NB are not read) and
 * only the diagonals j - i >= min_gap exist.  *found is always the exact number of runs; runs int32 [cap][3] holds them, sorted, when
 * found <= cap, and is unspecified otherwise (call again with a larger cap).  NA = 0 or NB = 0 finds nothing.  Refused before any
 * work: NA or NB outside 0 .. PVF_PRINT_MAX_ROWS, tau outside 0 .. 128, min_len < 1, self mode with min_gap < 1, cap < 0, null found,
 * null pointers where a count is positive.  PVF_RUNS_STRIP: the rows of A a workgroup of the kernel walks (what the tests' seams are
 * derived from). */
#define PVF_PRINT_MAX_ROWS 16777216      /* frames of one pvf_frame_prints call; rows of a table of pvf_print_runs */
#define PVF_RUNS_STRIP 1024
int32_t pvf_frame_prints(pvf_handle ctx, const pvf_handle* frames, int32_t n, uint64_t* out /* n*4 */, int32_t out_on_device);
int32_t pvf_print_runs(pvf_handle ctx, const uint64_t* A /* NA*2: H, V */, const uint8_t* usable_a, int32_t NA,
                       const uint64_t* B, const uint8_t* usable_b, int32_t NB,   /* B == NULL: self mode */
                       int32_t tau, int32_t min_len, int32_t min_gap,
                       int32_t* runs /* cap*3 */, int64_t cap, int64_t* found);

/* ---- fades and dissolves (BLEND.md; no reference call) ---------------------------------------------------------------------------
 * The blend record of a frame is a row of 16 uint32.  With G the tw x th thumbnail of the whole frame (the exact area average of the
 * storyboard's thumbnails), Y = (77 R + 150 G + 29 B + 128) >> 8 of it, P = tw th pixels: word 0 is P, words 1 .. 3 are S1 = sum Y,
 * S2 = sum Y^2 and E1 = sum |Y_t - Y_(t-1)|; words 4 .. 11 are E_L = sum |Y_t - Y_(t-L)| and R_L = sum |2 Y_(t-L/2) - Y_(t-L) - Y_t| for
 * L = 4, 8, 16, 32; words 12 and 13 are the caller's (written as 0), word 14 is tw | th << 16, word 15 is 0.  A sum whose earlier frame
 * does not exist is 0xFFFFFFFF.
 * The first call below measures n resident frames of one size.  hist holds the luma planes of the nh <= PVF_BLEND_MAX_HISTORY frames in
 * front of frames[0], oldest first; luma_out, when given, receives the planes of the n frames, of which the caller carries the last 32
 * into its next call.  The call keeps no state.  The second call measures rows first .. N - 1 of planes the caller made itself, with the
 * rows in front of them as history; S1 and S2 come from the planes and word 14 is 0.  n = 0, or first = N, does nothing.
 * Refused before any work: n, N or first negative, n beyond PVF_THUMB_MAX_FRAMES, N beyond PVF_BLEND_MAX_ROWS, first > N, nh outside
 * 0 .. 32, tw or th outside 1 .. PVF_THUMB_MAX_SIDE, P outside 1 .. PVF_BLEND_MAX_PIXELS, null pointers where a count is positive, an
 * unknown or released frame, frames of different sizes. */
#define PVF_BLEND_MAX_PIXELS 16384       /* tw * th: every sum of a row fits 32 bits */
#define PVF_BLEND_MAX_HISTORY 32         /* the largest lag */
#define PVF_BLEND_ROW_WORDS 16
#define PVF_BLEND_MAX_ROWS 16777216      /* planes of one call on planes */
int32_t pvf_frame_blend(pvf_handle ctx, const pvf_handle* frames, int32_t n, int32_t tw, int32_t th,
                        const uint8_t* hist /* nh*P, host */, int32_t nh, uint32_t* rows /* n*16, host */,
                        uint8_t* luma_out /* n*P host, or NULL */);
int32_t pvf_blend_measure(pvf_handle ctx, const uint8_t* luma /* N*P, host */, int32_t N, int32_t P, int32_t first,
                          uint32_t* rows /* (N-first)*16 */);

/* ---- camera motion from the shot detector's flow (MOTION.md; no reference call) ---------------------------------------------------
 * The motion row of a pair of frames is 10 int64.  The pair's flow, float32 [h][w][2] (component 0 horizontal, 1 vertical, small-image
 * pixels), is quantised to u, v in 1/64 pixel; a similarity u^ = TX + A X - B Y, v^ = TY + B X + A Y over the centred half-pixel
 * coordinates X = 2 x - (w - 1), Y = 2 y - (h - 1) is fitted by least squares in integers, then PVF_MOTION_ROUNDS - 1 more times over the
 * pixels whose residual lies within tau = max(PVF_MOTION_TAU_MIN, twice the mean residual) of the fit before.  Word 0 is
 * n_valid | n_in << 32; words 1 .. 4 are TX, TY, A, B scaled by 2^16; word 5 the mean residual m; word 6 the sum of |u| + |v| over the valid
 * pixels; word 7 the bits of the pair's displaced frame difference (0 from pvf_flow_motion); word 8 is the caller's (written as 0);
 * word 9 is w | h << 16.  MOTION.md states every step.
 * pvf_flow_motion fits n_pairs flows of the caller's (host).  pvf_shot_motion makes the small gray images and the flows of n resident
 * frames exactly as pvf_shot_dfd does (`tables` as there), fits the n - 1 flows where they lie on the device and returns the n - 1 rows,
 * and the n - 1 differences when dfd is not NULL; the flows do not leave the device.  n_pairs = 0 and n <= 1 do nothing.
 * Refused before any work: a negative count, a side outside PVF_MOTION_MIN_SIDE .. PVF_MOTION_MAX_SIDE, more than PVF_MOTION_MAX_PIXELS
 * pixels, null pointers where a count is positive, an unknown or released frame, frames of different sizes. */
#define PVF_MOTION_ROW_WORDS 10
#define PVF_MOTION_ROUNDS 4
#define PVF_MOTION_TAU_MIN (16 << 16)    /* 1/4 pixel, in the residual's unit of 2^-22 pixel */
#define PVF_MOTION_MIN_SIDE 12
#define PVF_MOTION_MAX_SIDE 256
#define PVF_MOTION_MAX_PIXELS 16384      /* w * h: every sum of the fit fits 64 bits */
#define PVF_MOTION_ROUND_PAIRS 256       /* pairs of pvf_flow_motion on the device at a time */
int32_t pvf_flow_motion(pvf_handle ctx, const float* flow /* n_pairs*h*w*2, host */, int32_t n_pairs, int32_t h, int32_t w,
                        int64_t* rows /* n_pairs*10, host */);
int32_t pvf_shot_motion(pvf_handle ctx, const pvf_handle* frames, int32_t n, int32_t width, int32_t height, const float* tables,
                        int64_t* rows /* (n-1)*10, host */, double* dfd /* n-1 host, or NULL */);

/* ---- overlaid text: the text record of a frame (CAPTION.md; no reference call) ------------------------------------------------------
 * On the luma Y = (77 R + 150 G + 29 B + 128) >> 8 of a resident h x w frame at full resolution, a pixel is a stroke pixel when the central
 * horizontal difference |Y(min(x + 1, w - 1), y) - Y(max(x - 1, 0), y)| is at least `edge`.  Per cell of PVF_TEXT_CELL x PVF_TEXT_CELL
 * pixels (cw = ceil(w / 16) by ch = ceil(h / 16); the right and lower cells may be partial): NP pixels inside the frame, E stroke pixels,
 * S stroke pixels that are stroke pixels of the predecessor too with |Y - Y_p| <= still, M pixels with |Y - Y_p| > still; without a
 * predecessor S = M = 0.  The predecessor of frames[i] is frames[i - 1], of frames[0] it is `prev` (0: none).  A row is uint32
 * [PVF_TEXT_HEAD_WORDS + ch * wpr], wpr = ceil(cw / 32): w | h << 16; edge | still << 8 | on << 16 | has_prev << 31; the sums of E, S and M
 * over the cells; the number of set bits; two words of the caller's (written as 0); then the mask, cell row r in words 8 + r * wpr ..,
 * cell c bit c & 31 of word c >> 5, the bit S >= on, bits at c >= cw 0.  counts, when not NULL, receives E, S, M, NP of every cell.
 * The call keeps no state: the caller hands the last frame of a batch in again as `prev` of the next.  n = 0 does nothing.
 * Refused before any work: n negative or beyond PVF_TEXT_MAX_FRAMES, edge outside 1 .. 255, still outside 0 .. 254, on outside
 * 1 .. 256, null frames or rows, an unknown or released frame (prev included), frames of different sizes, a side beyond PVF_TEXT_MAX_SIDE. */
#define PVF_TEXT_CELL 16
#define PVF_TEXT_HEAD_WORDS 8
#define PVF_TEXT_MAX_SIDE 8192
#define PVF_TEXT_MAX_FRAMES 4096
int32_t pvf_frame_text(pvf_handle ctx, const pvf_handle* frames, int32_t n, pvf_handle prev /* or 0 */,
                       int32_t edge, int32_t still, int32_t on,
                       uint32_t* rows   /* n * (8 + ch*wpr), host */,
                       uint16_t* counts /* n*ch*cw*4 = E, S, M, NP; host, or NULL */);

/* ---- what a person wears: colour histograms over windows of resident frames (CLOTHES.md; no reference call) -------------------------
 * The bin of a pixel (R, G, B): Y = (77 R + 150 G + 29 B + 128) >> 8, c1 = R - G, c2 = (2 B - R - G) >> 1 (an arithmetic shift: the floor),
 * q(c) = min(max((c + 64) >> 4, 0), 7), bin = (Y >> 6) * 64 + q(c1) * 8 + q(c2).  Window i is windows[4 i .. 4 i + 3] = (x0, y0, x1, y1)
 * of frame frames[i]: int32 pixels, half-open, anywhere relative to the frame; only pixels inside the frame count (the clip is computed in
 * 64 bits), x1 <= x0 or y1 <= y0 is an empty window.  Row y of a window belongs to band ((y - y0) * B) // (y1 - y0): the unclipped height.
 * out is uint32 [G][B][256]: the counts of all pixels of all windows i with group[i] = g, per band; a group without windows is zero.
 * Frames may differ in size within a call.  out: host memory, or with out_on_device device memory; the call is complete when it returns.
 * n = 0 writes zeros.  Windows go through the device as pieces, in rounds (2^18 pieces, or what the environment variable PVF_HIST_ROUND
 * names, read at the call); nothing depends on the rounds.
 * Refused before any work: n < 0 or beyond PVF_HIST_MAX_WINDOWS, G < 1, B outside 1 .. PVF_HIST_MAX_BANDS, G * B beyond PVF_HIST_MAX_ROWS,
 * null pointers with n > 0, a group outside 0 .. G - 1, an unknown or released frame, a group whose clipped pixels in this call number
 * 2^32 or more (the host adds the clipped areas in 64 bits before it launches). */
#define PVF_HIST_BINS 256
#define PVF_HIST_MAX_BANDS 4
#define PVF_HIST_MAX_WINDOWS 65536       /* windows of one call */
#define PVF_HIST_MAX_ROWS 65536          /* G * B: 64 MiB of result */
int32_t pvf_frame_hist(pvf_handle ctx, const pvf_handle* frames, const int32_t* windows /* n*4 */, const int32_t* group /* n */,
                       int32_t n, int32_t G, int32_t B, uint32_t* out /* G*B*256 */, int32_t out_on_device);

/* ---- file formats (host) ------------------------------------------------------------------------------ */
/* ref: scripts/pyannote-face.py:299-311  the lines of landmarks.txt / embedding.txt: "{t:.3f} {identifier:d}" + n_cols x " {v:.<decimals>f}"
 * + newline per row, byte for byte what Python's format writes (both are the correctly rounded decimal).  values [n_rows][n_cols];
 * out needs 64 + 42 * n_cols bytes per row; *written = bytes produced. */
int32_t pvf_format_rows(const double* t, const int64_t* identifier, const double* values, int64_t n_rows, int32_t n_cols,
                        int32_t decimals, char* out, int64_t cap, int64_t* written);

/* ref: scripts/pyannote-face.py:307-311, face/clustering.py:70-75  the float64 values `preprocess` reads back from the 5-decimal text of
 * embedding.txt, computed in memory: out[i] = rint((double)x[i] * 10^decimals) / 10^decimals (== np.round of the float64 value) */
int32_t pvf_round_rows(const float* x, int64_t n, int32_t decimals, double* out);

/* ref: face/clustering.py:70-75 (`read_table` of embedding.txt), scripts/pyannote-face.py:223-233 (track.txt)  whitespace-separated numeric
 * text -> float64 [n_rows][n_cols], row-major, the values strtod returns (one IEEE division for plain decimals of <= 15 digits, strtod for
 * the rest); rows of different lengths or a token that is not a number are errors.  cap = doubles `out` can hold (len / 2 + 1 suffices). */
int32_t pvf_parse_rows(const char* text, int64_t len, double* out, int64_t cap, int64_t* n_rows, int32_t* n_cols);

/* ---- measurement ----------------------------------------------------------------------------------- */
/* HIP-event timing of each kernel family on the context's stream ("pyramid","fhog","score","ert","chip","conv",
 * "dsst","pdist","hac"); off by default */
int32_t pvf_prof_enable(pvf_handle ctx, int32_t on);
int32_t pvf_prof_reset(pvf_handle ctx);
int32_t pvf_prof_get(pvf_handle ctx, const char* family, double* total_ms, int64_t* launches);

/* ---- stage access used by the parity tests ------------------------------------------------------------ */
int32_t pvf_debug_pyramid_level(pvf_handle ctx, pvf_handle frame, int32_t upsample, int32_t level,
                                uint8_t* out, int32_t* h, int32_t* w);               /* out may be NULL: dims only */
/* the image pyramids of a batch of frames and nothing else (the detector's resize chain alone, for measurements); returns when they are built */
int32_t pvf_debug_pyramid_batch(pvf_handle ctx, const pvf_handle* frames, int32_t n, int32_t upsample);
/* features of one pyramid level exactly as the batched detector computes them (all levels per launch); out [fh][fw][32] or NULL */
int32_t pvf_debug_level_features(pvf_handle ctx, pvf_handle frame, int32_t upsample, int32_t level,
                                 float* out, int32_t* fh, int32_t* fw);
/* how the plan of the frame's size cuts one level into pieces: out8 = level height, width, feature rows, feature columns, FHOG chunk
   height (feature rows), FHOG chunks, scoring piece height (output rows), scoring pieces */
int32_t pvf_debug_level_plan(pvf_handle ctx, pvf_handle frame, int32_t upsample, int32_t level, int32_t* out8);
int32_t pvf_debug_fhog(pvf_handle ctx, const uint8_t* img, int32_t h, int32_t w, int32_t cell, int32_t pad_r,
                       int32_t pad_c, float* out, int32_t* fh, int32_t* fw);          /* out [fh][fw][32] */
int32_t pvf_debug_detect_raw(pvf_handle ctx, pvf_handle frame, int32_t upsample, double adjust, float* scores,
                             int32_t* meta /* cap*8: filter,level,r,c,l,t,r,b */, int32_t cap, int32_t* n);
/* the same for any number of frames through the BATCHED path the engine runs (pvf_detect_many without its non-maximum suppression,
 * screening pass included): counts[n_frames]; rows [cap][5] = (level, filter, row, column, score bits) frame after frame in the
 * detector's canonical order; *total = all candidates (more than cap: only the first cap rows were written).  What the whole-clip
 * fixtures pin (tests/golden/c2_full.npz: the scanner's candidates before NMS, reference face.py:64-67). */
int32_t pvf_debug_detect_raw_many(pvf_handle ctx, const pvf_handle* frames, int32_t n_frames, int32_t batch, int32_t upsample,
                                  double adjust, int32_t* counts, int32_t* rows, int64_t cap, int64_t* total);
int32_t pvf_debug_extract_chip(pvf_handle ctx, pvf_handle frame, const double rect[4], double cs, double sn,
                               int32_t rows, int32_t cols, uint8_t* out);
int32_t pvf_debug_tracker_state(pvf_handle ctx, pvf_handle trk, double* F, double* A, double* B);
/* the scale filter of a started tracker: As [512][32][2] (index = (cell * 32 + plane), scale, re/im), Bs [32]; either may be NULL */
int32_t pvf_debug_tracker_scale_state(pvf_handle ctx, pvf_handle trk, double* As, double* Bs);
/* The embedder's forward as pvf_embed_chips runs it (split != 0: the f16 split path, without the exact second pass of flagged faces),
 * with the activation after `stage` copied out as out [n][dims[0]][dims[1]][dims[2]] fp32: stage 0 the first layer, 1 the max-pool,
 * 2 + 2u the `a` layer and 3 + 2u the output of residual unit u = 0..13 (30 stages; head_k, which averages and multiplies in one
 * kernel, is reached through pvf_debug_embed_head).  out == NULL: dims only, nothing runs.
 * flags [n] (may be NULL; split only): 1 for a face that left the f16 range.  n <= 4096. */
int32_t pvf_debug_embed_stage(pvf_handle ctx, const uint8_t* chips, int32_t n, int32_t split, int32_t stage, float* out, int32_t dims[3],
                              int32_t* flags);
/* ONE convolution layer (bias, affine, skip, ReLU) through the embedder's launcher on tensors of the caller, weights prepared by the
 * code the model loader uses.  geom = {B, H, W, Cin, OH, OW, Cout, AH, AW, ksz, stride, pad, skip_mode, XH, XW, XC, SH, SW}: in
 * [B][H][W][Cin], w [Cout][Cin][ksz][ksz], out [B][OH][OW][Cout] (conv results in [AH][AW], zero-extended), skip_mode 0 none,
 * 1 skip [B][OH][OW][Cout], 2 the 2 x 2 stride-2 average of skip [B][XH][XW][XC] added to [SH][SW] x the first XC channels.
 * split: the f16 split kernels where the product would use them, flags [B] (may be NULL) as above.  force_generic: never the
 * dedicated 35 x 35 x 32 kernel.  A shape the launcher does not take is an error; the context stays usable. */
int32_t pvf_debug_conv(pvf_handle ctx, const int32_t geom[18], const float* in, const float* w, const float* bias, const float* gamma,
                       const float* beta, const float* skip, int32_t split, int32_t force_generic, float* out, int32_t* flags);
/* head_k on x [n][hw][256] with the loaded model's 256 x 128 matrix: out [n][128] */
int32_t pvf_debug_embed_head(pvf_handle ctx, const float* x, int32_t n, int32_t hw, float* out);
/* The scratch arenas of the context (grow-only device buffers that the kernel families carve their intermediates from, several families
 * per arena).  report: one line "name capacity_in_bytes" per arena, NUL-terminated text; an arena that holds state across calls (the
 * detector's feature maps with their zero border, the resident ORB sets) has " state" behind its size.  *need is always the bytes of
 * the text with its NUL; the text is written only when cap >= *need (call again with that room; report may be NULL with cap 0).
 * fill = -1: report only.  fill = 0..255: both streams of the context are synchronised, the whole capacity of every arena that holds NO
 * state is set to that byte, and the device is synchronised again -- what a call then finds under its layout is what another family
 * could have left there.  Any other fill is refused before any work. */
int32_t pvf_debug_scratch(pvf_handle ctx, int32_t fill, char* report, int64_t cap, int64_t* need);

/* ---- f4: shot boundary detection ------------------------------------------------------------------
 * ref: pyannote/video/structure/shot.py:71-73 (_convert: RGB -> gray -> cv2.resize to `width` x `height`), :75-99 (dfd: Farneback flow
 *      with (0.5, 3, 15, 3, 5, 1.1, 0), per-pixel displaced lookup, mean absolute difference).  dfd[i] compares frames i and i + 1
 *      (n - 1 values).  tables = 22 floats (Gaussian g / x g / x^2 g for x = 0..5, then ig11, ig03, ig33, ig55: structure.shot_tables()).
 *      gray_out ([n][height][width] bytes) and flow_out ([n-1][height][width][2] floats) may be NULL.  The reference's default small
 *      image (50 pixels wide) has one pyramid level; a side of 64 pixels or more (Shot(height=...), shot.py:53-60) brings OpenCV's coarser
 *      levels -- up to three: halved while both sides stay >= 32 -- which run in the same launch. */
int32_t pvf_shot_dfd(pvf_handle ctx, const pvf_handle* frames, int32_t n, int32_t width, int32_t height, const float* tables,
                     double* dfd, uint8_t* gray_out, float* flow_out);

/* ---- shot threading (ORB.md) ------------------------------------------------------------------------------------
 * ref: pyannote/video/structure/thread.py:139-150 (_compute_orb: cv2.resize of the RGB frame to `width` x `height`, RGB -> gray,
 *      cv2.ORB_create().detectAndCompute with OpenCV 3.x defaults: 500 features, 1.2, 8 levels, edge 31, FAST 20, Harris, patch 31).
 *      For every frame: counts[i] keypoints, rows [i][cap][6] floats (x, y, level, FAST score, Harris response, angle in degrees;
 *      x and y in pixels of the keypoint's level) ordered by level, then y, then x, and descriptors [i][cap][32].  keypoints and
 *      descriptors may be NULL.  A frame with more than `cap` keypoints (retainBest keeps every point tied with the last one) is an
 *      error; cap is at most 65536.  On that error counts (if not NULL) is still written: counts[i] = -(keypoints of frame i) for
 *      every frame that does not fit, so the largest -counts[i] is the cap a second call needs; keypoints and descriptors are not
 *      written.  The descriptors stay on the device for pvf_orb_match_counts until the next call on this context; a call that
 *      fails leaves none. */
int32_t pvf_orb_extract(pvf_handle ctx, const pvf_handle* frames, int32_t n, int32_t width, int32_t height, int32_t cap,
                        int32_t* counts, float* keypoints, uint8_t* descriptors);
/* ref: thread.py:152-170 (_match: FlannBasedMatcher LSH knnMatch(k = 2), ratio 0.7) with an EXACT 2-nearest-neighbour search:
 *      counts[p] = the rows of set pairs[2p] whose best and second-best Hamming distances d1 <= d2 to the rows of set pairs[2p + 1]
 *      satisfy 10 d1 < 7 d2; 0 when either set has fewer than 2 rows.  descriptors ([n_sets][cap][32], rows[n_sets] of them used) ==
 *      NULL: the sets of the last pvf_orb_extract on this context (rows, n_sets and cap ignored). */
int32_t pvf_orb_match_counts(pvf_handle ctx, const uint8_t* descriptors, const int32_t* rows, int32_t n_sets, int32_t cap,
                             const int32_t* pairs, int64_t n_pairs, int32_t* counts);

#ifdef __cplusplus
}
#endif
#endif
