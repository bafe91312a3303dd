#!/usr/bin/env python
"""sha256 of the gfx950 code object of every entry of build.SOURCES.

    python scripts/device_code_digest.py [-o digests.json]

Each source is compiled with the exact line of build.build_native (PER_FILE_FLAGS and THR_EXTRA_CFLAGS
included) plus --offload-device-only, from the repository root with the relative path of the source, so
that two trees compile the same command.  One more option pins the compilation-unit id (-cuid=<source name>):
by default hipcc hashes it from the absolute paths of the source and of the output, which differ between two
trees and between two runs; the id names one symbol of the code object and appears in no instruction.  Two
trees whose digests are all equal run the same device code: what differs between them is host code.  Needs
hipcc, no GPU.
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from thrifty_amd import build  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("-o", "--out", help="also write the digests to this JSON file")
    ap.add_argument("-j", "--jobs", type=int, default=8)
    args = ap.parse_args()
    extra = os.environ.get("THR_EXTRA_CFLAGS", "").split()
    rel = os.path.relpath(build.CSRC, ROOT)
    digests = {}
    with tempfile.TemporaryDirectory() as tmp:
        todo = list(build.SOURCES)
        while todo:
            batch, todo = todo[:args.jobs], todo[args.jobs:]
            procs = []
            for src in batch:
                obj = os.path.join(tmp, src + ".co")
                cmd = build.compile_cmd(src, os.path.join(rel, src), obj, extra) + ["--offload-device-only", "-cuid=" + src]
                procs.append((src, obj, cmd, subprocess.Popen(cmd, cwd=ROOT)))
            for src, obj, cmd, proc in procs:
                if proc.wait() != 0:
                    raise subprocess.CalledProcessError(proc.returncode, cmd)
                with open(obj, "rb") as f:
                    digests[src] = hashlib.sha256(f.read()).hexdigest()
    for src in build.SOURCES:
        print(digests[src], src)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(digests, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
