"""Plain-NumPy restatement of the capture survey: np.bincount, integer sums, float32
samples -> float64 FFT -> abs.  `RefBackend` stands in for _native.Survey where there is no GPU."""
import numpy as np

C = np.float32(127.4)


def blocks_of(stream, block_len, history_len=0):
    """the overlapping u8 blocks [B, 2N] of a raw stream (block i starts 2 (N - H) i bytes in)"""
    buf = np.frombuffer(stream, dtype=np.uint8)
    step, blk = 2 * (block_len - history_len), 2 * block_len
    nb = 0 if len(buf) < blk else (len(buf) - blk) // step + 1
    return np.stack([buf[i * step:i * step + blk] for i in range(nb)]) if nb else np.zeros((0, blk), np.uint8)


def samples(blocks):
    """raw_to_complex: float32 (v - 127.4f) / 128, exact"""
    x = (blocks.astype(np.float32) - C) / np.float32(128)
    return x[:, 0::2].astype(np.float64) + 1j * x[:, 1::2].astype(np.float64)


def sums(blocks):
    b = blocks.astype(np.uint64)
    return np.stack([b.sum(axis=1), (b * b).sum(axis=1)], axis=1).astype(np.uint64)


def survey(blocks, integrate):
    """-> (mean_mag float64 [J, N], hist uint64 [J, 256], sums uint64 [B, 2]) over the whole intervals"""
    blocks = np.asarray(blocks, dtype=np.uint8)
    n_int = len(blocks) // integrate
    n = blocks.shape[1] // 2
    mean_mag = np.zeros((n_int, n))
    hist = np.zeros((n_int, 256), dtype=np.uint64)
    for j in range(n_int):
        part = blocks[j * integrate:(j + 1) * integrate]
        mean_mag[j] = np.abs(np.fft.fft(samples(part), axis=1)).mean(axis=0)
        hist[j] = np.bincount(part.ravel(), minlength=256)
    return mean_mag, hist, sums(blocks)


def energy(blocks):
    """sum |raw_to_complex(bytes)|^2 per block, float64"""
    x = samples(np.asarray(blocks, dtype=np.uint8))
    return (x.real ** 2 + x.imag ** 2).sum(axis=1)


class RefBackend(object):
    """_native.Survey's interface on the host: q = rint(|X| 2^S) from a float64 FFT, integer sums."""

    def __init__(self, block_len, history_len, integrate):
        self.block_len, self.history_len, self.integrate = block_len, history_len, integrate
        self.shift = 30 - int(np.log2(block_len))
        self.calls = []
        self.reset()

    def reset(self):
        self._open = np.zeros((0, 2 * self.block_len), dtype=np.uint8)

    def close(self):
        pass

    def feed(self, blocks, cap_intervals=None):
        blocks = np.asarray(blocks, dtype=np.uint8).reshape(-1, 2 * self.block_len)
        self.calls.append(("feed", len(blocks)))
        return self._fold(blocks)

    def feed_stream(self, stream, cap_intervals=None):
        blocks = blocks_of(stream, self.block_len, self.history_len)
        self.calls.append(("feed_stream", len(blocks)))
        return self._fold(blocks)

    def _fold(self, blocks):
        every = np.concatenate([self._open, blocks])
        k = self.integrate
        n_int = len(every) // k
        spec = np.zeros((n_int, self.block_len), dtype=np.uint64)
        hist = np.zeros((n_int, 256), dtype=np.uint64)
        for j in range(n_int):
            part = every[j * k:(j + 1) * k]
            q = np.rint(np.abs(np.fft.fft(samples(part), axis=1)) * 2.0 ** self.shift).astype(np.uint64)
            spec[j] = q.sum(axis=0)
            hist[j] = np.bincount(part.ravel(), minlength=256)
        self._open = every[n_int * k:]
        return spec, hist, sums(blocks)
