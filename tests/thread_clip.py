"""Test infrastructure: a small clip whose shots return to the same camera set-ups (A B A C B A by default): each set-up is a textured
scene (rectangles of random gray levels on low-pass noise), every frame a crop of it with a small camera jitter."""
import numpy as np

SETUPS = "ABACBA"


def _scene(seed, h, w):
    rng = np.random.default_rng(seed)
    small = rng.random((h // 16 + 2, w // 16 + 2, 3)) * 120 + 60
    img = np.repeat(np.repeat(small, 16, 0), 16, 1)[:h, :w].copy()
    for _ in range(40):
        rh, rw = rng.integers(8, h // 4), rng.integers(8, w // 4)
        y, x = rng.integers(0, h - rh), rng.integers(0, w - rw)
        img[y:y + rh, x:x + rw] = rng.integers(0, 256, 3)
    return img


def make_clip(width=480, height=270, frames_per_shot=20, setups=SETUPS, frame_rate=25.0, seed=7):
    """(frames uint8 [N, H, W, 3], shots [(start, end)] in seconds, frame_rate)"""
    pad = 8
    scenes = {k: _scene(seed * 100 + ord(k), height + 2 * pad, width + 2 * pad) for k in sorted(set(setups))}
    rng = np.random.default_rng(seed)
    frames = []
    for k in setups:
        for _ in range(frames_per_shot):
            dy, dx = rng.integers(-2, 3, 2)
            frames.append(scenes[k][pad + dy:pad + dy + height, pad + dx:pad + dx + width])
    n = frames_per_shot
    shots = [(i * n / frame_rate, (i + 1) * n / frame_rate) for i in range(len(setups))]
    return np.clip(np.stack(frames), 0, 255).astype(np.uint8), shots, frame_rate


class ClipVideo(object):
    """frames by index with the attributes Thread reads"""

    def __init__(self, frames, frame_rate):
        self._frames = frames
        self.frame_rate = frame_rate
        self._size = (frames.shape[2], frames.shape[1])
        self.step, self.start, self.end = 1.0 / frame_rate, 0.0, len(frames) / frame_rate

    def __len__(self):
        return len(self._frames)

    def frame(self, i):
        return np.ascontiguousarray(self._frames[i])

    def __call__(self, t):
        i = int(self.frame_rate * t + 0.00001)
        if not 0 <= i < len(self._frames):
            raise IOError("no frame at t = %.3f" % t)
        return self.frame(i)
