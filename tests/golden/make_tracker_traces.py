#!/usr/bin/env python3
"""Generates tests/golden/tracker_traces.json.gz: the trace of every scenario of tests/tracker_trace.py, as the
`SegmentTracker` of this tree makes it.  Needs no GPU and no built library.  Run it when the schedule is changed on
purpose, and review the difference (`zcat` of both, `diff`); a refactor leaves the file as it is.  Fixed gzip header
and sorted keys: a re-run on an unchanged tree gives the same bytes.
"""
import gzip
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import tracker_trace  # noqa: E402


class Environ:
    """`setenv` / `delenv` as pytest's monkeypatch has them."""
    @staticmethod
    def setenv(name, value):
        os.environ[name] = value

    @staticmethod
    def delenv(name, raising=True):
        os.environ.pop(name, None)


def main():
    traces = {key: tracker_trace.run(key, Environ) for key in tracker_trace.SCENARIOS}
    path = os.path.join(HERE, "tracker_traces.json.gz")
    with open(path, "wb") as f, gzip.GzipFile(filename="", fileobj=f, mode="wb", compresslevel=9, mtime=0) as z:
        z.write(json.dumps(traces, sort_keys=True, separators=(",", ":")).encode())
    print("%s: %d scenarios, %d entries, %d bytes" % (path, len(traces), sum(map(len, traces.values())),
                                                      os.path.getsize(path)))


if __name__ == "__main__":
    main()
