"""Stores what the reference's native block readers (oracle/_ref/libfastcard_readers.so, built by
oracle/Makefile) return for the inputs of tests/test_ref_readers.py and of the reference-reader tests of
tests/test_gpu_card_ingest.py and tests/test_gpu_card_tail.py -> tests/golden/ref_readers.npz, so that those tests also run where the
library cannot be built.  Needs the library (`make -C oracle`), no GPU:

    python tests/golden/make_golden_ref_readers.py
"""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
os.environ["THRIFTY_RECORD_REF"] = "1"

# the cases (test_ref_readers.ref_read's first argument) and the arrays stored per case, "<case>__<field>"
CASES = ["card_framing_64", "card_framing_4096", "card_framing_16384", "card_history_64", "card_history_0",
         "malformed_short", "malformed_long", "malformed_meta", "raw_64_16", "raw_4096_1024", "raw_16384_4920",
         "ingest_c2", "card_tail_64", "card_tail_128"]
FIELDS = ["sec", "usec", "idx", "data", "rc"]


def main():
    import numpy as np
    from oracle import ref_readers
    if not ref_readers.available():
        raise SystemExit("oracle/_ref/libfastcard_readers.so is not built: make -C oracle")
    # every case of tests/test_ref_readers.py, recorded by its own ref_read() calls (a fresh file)
    from test_ref_readers import STORED
    if os.path.exists(STORED):
        os.remove(STORED)
    subprocess.check_call([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider",
                           os.path.join(ROOT, "tests", "test_ref_readers.py")], cwd=ROOT)
    # the .card file of tests/test_gpu_card_ingest.py::test_device_ingest_equals_the_reference_native_card_reader
    from test_gpu_detector_api import card_text
    from test_ref_readers import ref_read
    g = np.load(os.path.join(ROOT, "tests", "golden", "c2.npz"), allow_pickle=False)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "rx.card")
        with open(path, "w") as f:
            f.write("# capture\n" + card_text(g))
        ref_read("ingest_c2", path, int(g["block_len"]), int(g["history_len"]), card=True)
        # the planted tails of tests/test_gpu_card_tail.py::test_the_reference_native_reader_decodes_the_same_bytes
        from test_gpu_card_tail import ref_reader_case
        for n in (64, 128):
            case, path, _ = ref_reader_case(n, d)
            ref_read(case, path, n, 0, card=True)
    have = sorted(np.load(STORED).files)
    assert have == sorted("%s__%s" % (c, f) for c in CASES for f in FIELDS), have


if __name__ == "__main__":
    main()
