"""`python -m thrifty_amd.template_generate LENGTH [INDEX] [-o template.npy]` -- the base template of a
transmitter's Gold code, sampled at sample_rate / chip_rate samples per chip (integer sampler, no
filter): the first step of producing a receiver's template (then `thrifty_amd.template_extract`).
Host only; the code family is `thrifty_amd.synth`'s."""
from __future__ import annotations

import argparse
import sys

import numpy as np

from thrifty_amd import synth
from thrifty_amd.settings import load_args

SUMMARY = ("Generated new template: {symbols} symbols @ {chip_mhz:.6f} MHz = {ms:.3f} ms "
           "--> {samples} samples @ {msps:.6f} Msps")


def summary(nbits, n_samples, sample_rate, chip_rate):
    """The sentence the reference prints for a generated template."""
    symbols = (1 << nbits) - 1
    return SUMMARY.format(symbols=symbols, chip_mhz=chip_rate / 1e6, ms=symbols / chip_rate * 1e3,
                          samples=n_samples, msps=sample_rate / 1e6)


def build_parser():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("length", type=int, help="register length n of the Gold code: 2^n - 1 chips")
    parser.add_argument("index", type=int, nargs="?", default=0, help="which code of that family [default: 0]")
    parser.add_argument("-o", "--output", default="template.npy", help="where the .npy goes [default: template.npy]")
    return parser


def main(argv=None):
    config, args = load_args(build_parser(), ["sample_rate", "chip_rate"], argv=argv)
    template = synth.gold_template(args.length, args.index, config.sample_rate / config.chip_rate)
    np.save(args.output, template)
    print(summary(args.length, len(template), config.sample_rate, config.chip_rate))
    return 0


if __name__ == "__main__":
    sys.exit(main())
