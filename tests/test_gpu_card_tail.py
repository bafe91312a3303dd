"""The base64 ingest kernel (k_b64_decode, csrc/card_ingest.hip) at every tail and thread seam.

A block of N samples is 2N bytes and N is a power of two, so 2N is never a multiple of 3: the last
base64 quantum of a payload yields 2 bytes (one `=`) when log2 N is even and 1 byte (`==`) when it is
odd.  The other suites send .card text of 16384- and 4096-sample blocks through the engine -- both
the 2-byte tail; the `remaining == 1` branch of the kernel, its padding rule (`=` in the third
character is legal there and only there) and its store guards are what 128, 512, 2048, 8192, 32768,
131072 and 524288 take.  The thread layout has extremes of its own: one workgroup with 11 live
threads (N = 64) up to 683 workgroups per line (N = 2^20); the last live thread holds 3 quanta with
the 2-byte tail and 2 with the 1-byte tail; every thread before it stores three aligned dwords,
the last one stores bytes.

The engine exposes no decoded bytes, only records.  So per block length: one synthetic block, and
for every planted byte position p -- the last three bytes, the first 12, the 12 around the switch
from dword-storing threads to the last live thread, the 12 around the first and the last workgroup
boundary (byte 3 * 4 * 256 * k) -- two copies of it, with 0 and with 255 at p; the same for the
planted groups (the last one, two, three bytes and each 12-byte stretch as a whole).  The text is
made with Python's `base64`, in lines whose header widths put the payload on every residue mod 16
(the kernel loads 16 characters per thread from an arbitrary address).  detect_card(text) must equal
detect(bytes) BYTE FOR BYTE, and the host-path records of the two copies must DIFFER -- otherwise
the comparison could not have seen that byte, and the row fails.

  (a) without a GPU: launch_b64_decode's arithmetic restated; the table's claims; both tails, both
      last-thread counts, one workgroup per line and 683 are present; the planted positions sit where
      they claim; the lines decode to the blocks; the reference's own native reader (oracle/_ref,
      test_ref_readers.ref_read) decodes the accepted lines of the two smallest lengths to the same bytes
  (b) every row: text path == byte path, each planted byte visible; one row through thr_run_card
  (c) rejections, one length of each tail: NativeError, and the engine still works afterwards

Seeded mutations on scratch builds of the byte-storing branch (both stay in bounds): applying the
2-byte tail's padding rule `c & 0xC0u` to every tail refuses every `==` line -- the six 1-byte-tail
rows, the thr_run_card row and the 8192 rejection row fail, test_gpu_card_ingest.py and
test_gpu_run_file.py pass; storing `v >> 8` as a tail quantum's first byte fails every row here and
is also seen by those two files (the last live thread holds three quanta at 16384 and 4096)."""
import base64

import numpy as np
import pytest

from oracle import thrifty_np as onp
from thrifty_amd import _native as F
from thrifty_amd import block_data, synth

THREADS = 256                      # k_b64_decode's workgroup
QUANTA_PER_THREAD = 4              # 16 characters in, 12 bytes out
WG_BYTES = 3 * QUANTA_PER_THREAD * THREADS
MAX_BATCH = 7                      # far fewer than the lines of a row: several chunks per call


def layout(n):
    """launch_b64_decode / k_b64_decode restated -> dict(tail, n_quanta, threads, blocks_per_line,
    last_thread_quanta)."""
    out_bytes = 2 * n
    n_quanta = (out_bytes + 2) // 3
    threads = (n_quanta + 3) // 4
    return dict(tail=out_bytes - 3 * (n_quanta - 1), n_quanta=n_quanta, threads=threads,
                blocks_per_line=(threads + THREADS - 1) // THREADS,
                last_thread_quanta=n_quanta - QUANTA_PER_THREAD * (threads - 1))


# block length -> (bytes of the last quantum, n_quanta, blocks_per_line, quanta of the last live thread)
TABLE = {
    64: (2, 43, 1, 3),                  # the smallest block: one workgroup, 11 live threads
    128: (1, 86, 1, 2),
    512: (1, 342, 1, 2),
    1024: (2, 683, 1, 3),               # control: the tail the other suites cover
    2048: (1, 1366, 2, 2),
    8192: (1, 5462, 6, 2),              # the length of the reference's own tests
    32768: (1, 21846, 22, 2),
    131072: (1, 87382, 86, 2),
    1 << 20: (2, 699051, 683, 3),       # the largest block: 683 workgroups per line
}

# block length -> (template, history, carrier window, carrier bins of the planted tone, thresholds)
def geometry(n):
    if n == 64:
        tpl = np.sign(np.random.default_rng(4).normal(0, 1, 15))
        return tpl, len(tpl) + 8, (2, 14), (3.2, 12.0), (0, 8, 0)
    bits, sps, h, cwin = {128: (5, 1, 38, (2, 28)), 512: (6, 1, 62, (3, 60)), 1024: (7, 1, 256, (3, 60)),
                          2048: (8, 1, 512, (5, 100)), 8192: (10, 1, 2048, (7, 110)),
                          32768: (10, 1, 4096, (7, 110)), 131072: (11, 1, 4096, (7, 110)),
                          1 << 20: (11, 2, 4096, (7, 110))}[n]
    tpl = synth.gold_template(bits, 2, float(sps)).astype(np.float64)
    return tpl, h, cwin, (cwin[0] + 3.0, min(cwin[1] - 5.0, n / 8.0)), (0, 15, 0)


def stretches(n):
    """name -> the byte positions of one planted stretch of a 2N-byte block."""
    lay = layout(n)
    nbytes = 2 * n
    switch = 12 * (lay["threads"] - 1)          # first byte of the last live thread (which stores bytes)
    out = {"last1": [nbytes - 1], "last2": [nbytes - 2, nbytes - 1], "last3": [nbytes - 3, nbytes - 2, nbytes - 1],
           "first12": list(range(12)), "switch12": list(range(switch - 6, min(switch + 6, nbytes)))}   # (the last thread holds 4 or 8 bytes)
    if lay["blocks_per_line"] > 1:
        out["wg_first12"] = list(range(WG_BYTES - 6, WG_BYTES + 6))
        k = lay["blocks_per_line"] - 1
        if k > 1:
            out["wg_last12"] = list(range(WG_BYTES * k - 6, WG_BYTES * k + 6))
    assert all(0 <= p < nbytes for s in out.values() for p in s)
    return out


def plants(n):
    """Every planted position set of a row: each single byte of every stretch, then the stretches as
    groups -> list of (name, positions)."""
    st = stretches(n)
    singles = sorted({p for s in st.values() for p in s})
    return [("byte%d" % p, [p]) for p in singles] + [(k, v) for k, v in st.items() if len(v) > 1]


def base_block(n):
    tpl, h, cwin, car, thr = geometry(n)
    rng = np.random.default_rng(3000 + n)
    blocks, _ = synth.synth_blocks(rng, 1, n, tpl, onp.unique_window(n, h, len(tpl)), signal_frac=1.0,
                                   carrier_bins=car)
    return blocks[0]


def planted_blocks(n):
    """-> u8 [2 * len(plants), 2N]: per plant the base block with 0 and with 255 on its positions."""
    base = base_block(n)
    pl = plants(n)
    out = np.empty((2 * len(pl), 2 * n), dtype=np.uint8)
    for j, (_, pos) in enumerate(pl):
        out[2 * j] = base
        out[2 * j + 1] = base
        out[2 * j, pos] = 0
        out[2 * j + 1, pos] = 255
    return out


def card_lines(blocks, comment=True):
    """.card text of `blocks` made with Python's base64; header widths chosen so that the payload of
    line k starts on residue k mod 16 -> (text bytes, payload offsets, block indices, timestamps)."""
    parts, offs, idxs, stamps = [], [], [], []
    pos = 0
    if comment:
        parts.append(b"# planted tails\n")
        pos = len(parts[0])
    for k, blk in enumerate(blocks):
        total = 11 + ((k % 16) - pos - 11) % 16            # header characters: 11 .. 26
        d_sec = min(10, total - 9 - 1)
        d_idx = total - 9 - d_sec
        sec = 10 ** (d_sec - 1) + k
        idx = 10 ** (d_idx - 1) + 3 * k if d_idx > 1 else k % 10
        usec = (k * 7919) % 1000000
        head = b"%d.%06d %d " % (sec, usec, idx)
        assert len(head) == total
        line = head + base64.b64encode(blk.tobytes()) + b"\n"
        offs.append(pos + len(head))
        idxs.append(idx)
        stamps.append((sec, usec))
        parts.append(line)
        pos += len(line)
    return b"".join(parts), np.asarray(offs, dtype=np.int64), np.asarray(idxs, dtype=np.int64), stamps


# ---------------------------------------------------------------------------------------------
# (a) without a GPU
# ---------------------------------------------------------------------------------------------
def test_the_table_restates_the_launch_arithmetic():
    for n, (tail, n_quanta, bpl, last_q) in TABLE.items():
        lay = layout(n)
        assert (lay["tail"], lay["n_quanta"], lay["blocks_per_line"], lay["last_thread_quanta"]) == (
            tail, n_quanta, bpl, last_q), n
        log2 = n.bit_length() - 1
        assert 1 << log2 == n and tail == (2 if log2 % 2 == 0 else 1)
        # the payload Python writes: n_quanta quanta, 3 - tail `=` at the end
        text = base64.b64encode(bytes(2 * n))
        assert len(text) == 4 * n_quanta == ((2 * n + 2) // 3) * 4          # (CardStream.payload_chars)
        assert text.endswith(b"=" * (3 - tail)) and not text.endswith(b"=" * (4 - tail))
        # the last live thread takes the byte-storing branch; every thread before it is `whole`
        q0_last = 4 * (lay["threads"] - 1)
        assert not (q0_last + 4 <= n_quanta and 2 * n - 3 * q0_last >= 12)
        q0_prev = q0_last - 4
        assert q0_prev + 4 <= n_quanta and 2 * n - 3 * q0_prev >= 12 and (2 * n) % 4 == 0


def test_the_table_covers_both_tails_and_both_layout_extremes():
    assert {64, 128, 512, 2048, 8192, 32768, 131072, 1 << 20} <= set(TABLE)
    assert {1024, 16384} & set(TABLE)                                  # a control with the covered tail
    parities = {(n.bit_length() - 1) % 2 for n in TABLE}
    assert parities == {0, 1}
    assert {t[0] for t in TABLE.values()} == {1, 2}
    assert {t[3] for t in TABLE.values()} == {2, 3}
    # powers of two produce no other last-thread count (64 .. 2^20), and the tail decides it
    for log2 in range(6, 21):
        lay = layout(1 << log2)
        assert (lay["tail"], lay["last_thread_quanta"]) in ((2, 3), (1, 2))
    bpls = [t[2] for t in TABLE.values()]
    assert min(bpls) == 1 and max(bpls) == 683 and TABLE[64][2] == 1 and layout(64)["threads"] == 11
    assert layout(1024)["blocks_per_line"] == 1 and layout(2048)["blocks_per_line"] == 2


@pytest.mark.parametrize("n", list(TABLE))
def test_the_planted_positions_sit_on_the_seams(n):
    lay, st = layout(n), stretches(n)
    nbytes = 2 * n
    assert st["last3"] == [nbytes - 3, nbytes - 2, nbytes - 1] and st["first12"][0] == 0
    # the last quantum holds `tail` bytes: last1 .. last3 reach into the quantum before it
    first_of_last_quantum = 3 * (lay["n_quanta"] - 1)
    assert nbytes - first_of_last_quantum == lay["tail"] and st["last3"][0] < first_of_last_quantum
    # the switch: bytes on both sides of the last live thread's first byte
    sw = 12 * (lay["threads"] - 1)
    assert st["switch12"][0] < sw <= st["switch12"][-1] and sw + 3 * lay["last_thread_quanta"] - (3 - lay["tail"]) == nbytes
    if lay["blocks_per_line"] > 1:
        assert st["wg_first12"][6] == WG_BYTES                  # thread 0 of workgroup 1 starts here
        assert WG_BYTES // 12 == THREADS
    if lay["blocks_per_line"] > 2:
        assert st["wg_last12"][6] == WG_BYTES * (lay["blocks_per_line"] - 1) < nbytes
    pl = plants(n)
    names = [p[0] for p in pl]
    assert len(set(names)) == len(names) and {"last2", "last3", "first12", "switch12"} <= set(names)
    assert {"byte%d" % (nbytes - k) for k in (1, 2, 3)} <= set(names)


@pytest.mark.parametrize("n", [64, 128, 512, 1024, 2048])
def test_the_lines_decode_to_the_blocks_and_meet_every_residue(n):
    blocks = planted_blocks(n)
    text, offs, idxs, stamps = card_lines(blocks)
    chars = 4 * layout(n)["n_quanta"]
    assert len(blocks) > 2 * MAX_BATCH and set((offs % 16).tolist()) == set(range(16))
    for k in range(len(blocks)):
        pay = bytes(text[offs[k]:offs[k] + chars])
        assert text[offs[k] + chars:offs[k] + chars + 1] == b"\n" and text[offs[k] - 1:offs[k]] == b" "
        assert base64.b64decode(pay, validate=True) == blocks[k].tobytes()
    # each pair differs exactly on its planted positions, which hold 0 and 255
    for j, (_, pos) in enumerate(plants(n)):
        diff = np.flatnonzero(blocks[2 * j] != blocks[2 * j + 1])
        assert diff.tolist() == sorted(pos) and (blocks[2 * j, pos] == 0).all() and (blocks[2 * j + 1, pos] == 255).all()
    # the product's own framing finds the same payloads and header fields
    import io
    got = block_data.CardStream(io.BytesIO(text), n).next_batch(10000)
    assert np.array_equal(got[3], offs) and np.array_equal(got[1], idxs)
    assert [round(t * 1e6) for t in got[0]] == [s * 1000000 + u for s, u in stamps]


REF_LINES = 6


def ref_reader_case(n, directory):
    """The accepted lines the reference's native reader is asked about: the first and the last
    REF_LINES / 2 planted blocks of a row (the first 12 bytes, the last three) -> (case, path, blocks)."""
    blocks = planted_blocks(n)
    blocks = np.concatenate([blocks[:REF_LINES // 2], blocks[-(REF_LINES - REF_LINES // 2):]])
    text, _, _, _ = card_lines(blocks)
    path = "%s/tail_%d.card" % (directory, n)
    with open(path, "wb") as f:
        f.write(text)
    return "card_tail_%d" % n, path, blocks


@pytest.mark.parametrize("n", [64, 128])
def test_the_reference_native_reader_decodes_the_same_bytes(tmp_path, n):
    """fastcard/card_reader.c + lib/base64.c (oracle/_ref where it is built, its stored output where it
    cannot be: test_ref_readers.ref_read) on the accepted lines of either tail == Python's base64."""
    from test_ref_readers import ref_read
    case, path, blocks = ref_reader_case(n, str(tmp_path))
    text, offs, idxs, stamps = card_lines(blocks)
    ref, rc = ref_read(case, path, n, 0, card=True)
    assert rc == 1 and len(ref) == REF_LINES
    chars = 4 * layout(n)["n_quanta"]
    for k, (sec, usec, idx, data) in enumerate(ref):
        assert (sec, usec) == stamps[k] and idx == idxs[k]
        want = np.frombuffer(base64.b64decode(text[offs[k]:offs[k] + chars], validate=True), dtype=np.uint8)
        assert np.array_equal(data, want) and np.array_equal(data, blocks[k])
    assert {layout(m)["tail"] for m in (64, 128)} == {1, 2}


# ---------------------------------------------------------------------------------------------
# (b) the text path against the byte path, on a GPU
# ---------------------------------------------------------------------------------------------
def engine_of(n):
    tpl, h, cwin, _, thr = geometry(n)
    return F.Engine(n, h, tpl, thr, cwin, thr, max_batch=MAX_BATCH)


def fields_differ(a, b, skip=("block_idx", "reserved")):
    return any(a[f] != b[f] for f in a.dtype.names if f not in skip)


def assert_every_plant_is_visible(n, rec_host):
    """The records of the copy with 0 and of the copy with 255 on a planted position differ: the
    byte-for-byte comparison of the two paths can see that position."""
    blind = [name for j, (name, _) in enumerate(plants(n)) if not fields_differ(rec_host[2 * j], rec_host[2 * j + 1])]
    assert not blind, "block length %d: planted bytes that change no record field: %s" % (n, blind)


@pytest.mark.gpu
@pytest.mark.parametrize("n", list(TABLE))
def test_text_path_equals_byte_path_at_every_tail_and_seam(n):
    blocks = planted_blocks(n)
    text, offs, idxs, _ = card_lines(blocks)
    assert len(blocks) > 2 * MAX_BATCH and set((offs % 16).tolist()) == set(range(16))
    eng = engine_of(n)
    rec_host = eng.detect(blocks, idxs)
    rec_card = eng.detect_card(text, offs, idxs)
    assert np.array_equal(rec_host["block_idx"][:, 0], idxs)
    assert rec_card.tobytes() == rec_host.tobytes()
    assert_every_plant_is_visible(n, rec_host[:, 0])
    eng.close()


@pytest.mark.gpu
def test_run_card_reaches_the_one_byte_tail_by_its_own_loop():
    """thr_run_card frames the text itself and submits chunk by chunk: the same kernel, another caller.
    Its record sink holds the detections only (timestamp bits in `reserved`)."""
    n = 8192
    assert TABLE[n][0] == 1
    blocks = planted_blocks(n)
    text, offs, idxs, stamps = card_lines(blocks)
    eng = engine_of(n)
    rec_host = eng.detect(blocks, idxs)[:, 0]
    det = (rec_host["flags"] & F.FLAG_CORR) != 0
    assert det.sum() > 0.9 * len(blocks)                            # the sink sees (nearly) every planted block
    assert_every_plant_is_visible(n, rec_host)
    sink = np.zeros(len(blocks), dtype=F.RECORD_DTYPE)
    st = eng.run_card(text, rec_out=sink)
    assert st["blocks"] == len(blocks) and st["detections"] == det.sum() and not st["index_error"]
    got, want = sink[:det.sum()], rec_host[det]
    for f in F.RECORD_DTYPE.names:
        if f != "reserved":
            assert np.array_equal(got[f], want[f]), f
    ts = np.asarray([s + u * 1e-6 for s, u in stamps])[det]
    assert np.array_equal(got["reserved"].view(np.float64), ts)
    eng.close()


# ---------------------------------------------------------------------------------------------
# (c) rejections
# ---------------------------------------------------------------------------------------------
def one_line(n):
    blk = base_block(n)
    head = b"12.000500 77 "
    return head, base64.b64encode(blk.tobytes()), blk


def bad_payloads(n):
    """name -> payload that must be refused, for the tail this length has."""
    _, pay, _ = one_line(n)
    lay = layout(n)
    L = len(pay)

    def put(at, ch):
        return pay[:at] + ch + pay[at + 1:]
    out = {"pad_in_second_to_last_quantum": put(L - 5, b"="),
           "pad_in_second_to_last_quantum_third_char": put(L - 6, b"="),
           "invalid_in_last_full_group": put(16 * (lay["threads"] - 2) + 5, b"!"),
           "invalid_in_first_group": put(2, b"\x80")}
    for k in range(4):
        out["invalid_in_last_quantum_char%d" % k] = put(L - 4 + k, b"*")
    if lay["tail"] == 1:
        assert pay.endswith(b"==") and pay[-3:-2] != b"="
        out["pad_in_second_char"] = put(L - 3, b"=")              # `X===`: position 1 is never padding
        out["pad_in_first_char"] = put(L - 4, b"=")
    else:
        assert pay.endswith(b"=") and pay[-2:-1] != b"="
        out["two_pads_on_a_two_byte_tail"] = put(L - 2, b"=")     # `XX==` where `XXX=` is due
        out["pad_in_second_char"] = put(L - 3, b"=")
    assert all(len(v) == L and v != pay for v in out.values())
    return out


REJECT_LENGTHS = [8192, 1024]           # the 1-byte tail (6 workgroups per line) and the 2-byte tail


def test_the_rejection_rows_are_what_they_claim():
    assert [TABLE[n][0] for n in REJECT_LENGTHS] == [1, 2]
    for n in REJECT_LENGTHS:
        _, pay, blk = one_line(n)
        assert base64.b64decode(pay, validate=True) == blk.tobytes()
        bad = bad_payloads(n)
        assert len(bad) >= 10 and {"invalid_in_last_quantum_char%d" % k for k in range(4)} <= set(bad)
        # the legal padding of this tail: `=` in the third character only with the 1-byte tail
        assert (pay[-2:-1] == b"=") == (TABLE[n][0] == 1) and pay[-1:] == b"="
        lay = layout(n)
        at = 16 * (lay["threads"] - 2) + 5
        assert at // 16 == lay["threads"] - 2 and at < len(pay) - 4 * lay["last_thread_quanta"]


@pytest.mark.gpu
@pytest.mark.parametrize("n", REJECT_LENGTHS)
def test_bad_tails_are_rejected_and_the_engine_goes_on(n):
    head, pay, blk = one_line(n)
    eng = engine_of(n)
    want = eng.detect(blk[None, :], np.asarray([77]))
    good = head + pay + b"\n"
    offs = np.asarray([len(head)], dtype=np.int64)
    assert eng.detect_card(good, offs, np.asarray([77])).tobytes() == want.tobytes()
    for name, bad in bad_payloads(n).items():
        # the bad line alone, and between two good ones (a call is refused as a whole)
        for text, o in ((head + bad + b"\n", offs),
                        (good + head + bad + b"\n" + good, np.asarray([len(head) + k * len(good) for k in range(3)]))):
            with pytest.raises(F.NativeError):
                eng.detect_card(text, o, np.full(len(o), 77))
            assert eng.detect_card(good, offs, np.asarray([77])).tobytes() == want.tobytes(), name
    eng.close()
