"""One front end for the package's commands: `python -m thrifty_amd.cli <command> [args]`.

The counterpart of the reference's `thrifty <command>`.  Every command is a module with its own argument
parser; `help <command>` shows it.  The capture, plot and analysis commands of the reference need radio
hardware or a display and are not part of this port: they are named, answered with one sentence and
exit status 1, like a command nobody knows.
"""
from __future__ import print_function

import importlib
import sys

# command -> (module, function that takes the argument list, one line for `help`)
COMMANDS = {
    "detect": ("thrifty_amd.cli", "_detect", "Detect presence of positioning signals and estimate SoA"),
    "identify": ("thrifty_amd.identify", "_main", "Identify transmitter IDs and filter duplicate detections"),
    "match": ("thrifty_amd.matchmaker", "_main", "Match detections from multiple receivers"),
    "tdoa": ("thrifty_amd.tdoa_est", "_main", "Estimate TDOA by synchronising with beacon transmissions"),
    "pos": ("thrifty_amd.pos_est", "_main", "Estimate position from TDOA estimates"),
    "locate": ("thrifty_amd.kitchen_sink", "_main", "identify, match, tdoa and pos in one device call"),
    "template_generate": ("thrifty_amd.template_generate", "main", "Generate a new (ideal) template"),
    "template_extract": ("thrifty_amd.template_extract", "main", "Extract a new template from captured data"),
}
NOT_PORTED = ("capture", "scope", "analyze_toads", "analyze_detect", "analyze_beacon", "analyze_tdoa")


def _detect(argv):
    from thrifty_amd import detect, detect_cli
    return detect_cli.detector_cli(detect.Detector, argv=argv)


def usage():
    lines = ["usage: python -m thrifty_amd.cli <command> [<args>]", "", "Commands:", ""]
    lines += ["    %-18s%s" % (name, COMMANDS[name][2]) for name in COMMANDS]
    lines += ["", "Not part of this port (capture hardware, plots, analysis): " + ", ".join(NOT_PORTED) + ".", "",
              "'help <command>' shows a command's arguments."]
    return "\n".join(lines)


def resolve(command):
    """The callable behind a command; it takes the list of the command's arguments."""
    module, function, _ = COMMANDS[command]
    return getattr(importlib.import_module(module), function)


def main(argv=None):
    """Runs one command and returns the exit status (a command's own SystemExit passes through)."""
    argv = list(sys.argv[1:] if argv is None else argv)
    if not argv:
        print(usage())
        return 1
    command, rest = argv[0], argv[1:]
    if command in ("help", "--help", "-h"):
        if not rest:
            print(usage())
            return 0
        command, rest = rest[0], ["--help"]
    if command in NOT_PORTED:
        print("thrifty_amd: '%s' is not part of this port (it needs capture hardware or a display)." % command,
              file=sys.stderr)
        return 1
    if command not in COMMANDS:
        print("thrifty_amd: '%s' is not a command. See 'python -m thrifty_amd.cli help'." % command, file=sys.stderr)
        return 1
    program = sys.argv[0]
    sys.argv[0] = "%s %s" % (program, command)      # the command's parser names itself after it
    try:
        status = resolve(command)(rest)
    finally:
        sys.argv[0] = program
    return 0 if status is None else status


if __name__ == "__main__":
    sys.exit(main())
