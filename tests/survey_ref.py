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


def tone_bin(b, n):
    """the bin of block b's tone.  5 is odd and n / 2 a power of two, so any n / 2 consecutive blocks have
    n / 2 different bins"""
    return (3 + 5 * b) % (n // 2)


def signature_amplitude(n):
    """the tone's amplitude in LSB: 40, and 100 below 4096, where 40 leaves the K-th tone bin of K = 5
    less than four times the largest other bin (measured 2.35 at 64 and 3.41 at 1024)"""
    return 40.0 if n >= 4096 else 100.0


def signature_tail(n):
    """bytes at a block's end that hold its constant: 64, and n / 32 below 2048.  A constant far from
    127.4 over T bytes puts 0.35 T |v - 127.4| / 128 into bin 0 and a step's leakage into every bin; with
    64 bytes at n = 64 (half the block) that is 45 beside a full-scale tone's 29, so no amplitude a byte
    can hold passes the top-K assertion there (measured ratio 0.19 at amplitude 110, K = 5)"""
    return min(64, n // 32)


def signature_blocks(nb, n, seed):
    """A scene in which every block says which one it is, twice: block b is noise of 10 LSB around 127.4
    plus a tone of signature_amplitude(n) LSB on bin tone_bin(b, n) (the spectrum's signature), and its last
    signature_tail(n) bytes are the constant (7 b + 1) mod 256 (the histogram's).  -> u8 [nb, 2 n]"""
    window = min(nb, n // 2)
    bins = np.array([tone_bin(b, n) for b in range(nb)])
    for lo in range(nb - window + 1):       # any K <= n / 2 consecutive blocks: K different bins
        assert len(np.unique(bins[lo:lo + window])) == window, (n, lo)
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)
    amp, tail = signature_amplitude(n), signature_tail(n)
    out = np.empty((nb, 2 * n), dtype=np.uint8)
    for b in range(nb):
        z = amp * np.exp(2j * np.pi * bins[b] * t / n)
        iq = np.stack([z.real, z.imag], axis=1).ravel() + 10.0 * rng.standard_normal(2 * n) + 127.4
        out[b] = np.clip(np.rint(iq), 0, 255)
        out[b, 2 * n - tail:] = (7 * b + 1) % 256
    return out


def tone_bins(j, k, n):
    """the sorted tone bins of interval j's blocks j k ... j k + k - 1, counted from the first block fed"""
    assert k <= n // 2
    return sorted(tone_bin(b, n) for b in range(j * k, (j + 1) * k))


def top_bins(row, k):
    """the sorted indices of the k largest entries of a spectrum row"""
    row = np.asarray(row)
    return sorted(np.argpartition(row, len(row) - k)[-k:].tolist())


def tone_margin(row, j, k, n):
    """the smallest tone bin of interval j over the largest bin that holds no tone"""
    bins = tone_bins(j, k, n)
    row = np.asarray(row, dtype=np.float64)
    return float(row[bins].min() / np.delete(row, bins).max())


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
