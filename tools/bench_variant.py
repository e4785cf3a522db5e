#!/usr/bin/env python3
"""bench.py under a named variant of the library (icelk_set_variant), without editing bench.py: every Context the run
creates gets the variants set right after it is made, the way the tests set them.

    python tools/bench_variant.py lk_wide_sums=1 -- --steps 200 --dump-outputs D

The rate of such a run is a measurement of the variant, never the headline."""
import os
import runpy
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    if "--" not in sys.argv:
        raise SystemExit(__doc__)
    cut = sys.argv.index("--")
    variants = [a.split("=") for a in sys.argv[1:cut]]
    from iceberg_tracking_code_amd import context
    init = context.Context.__init__

    def patched(self, *a, **kw):
        init(self, *a, **kw)
        for name, value in variants:
            self.set_variant(name, int(value))

    context.Context.__init__ = patched
    sys.argv = [os.path.join(ROOT, "bench.py")] + sys.argv[cut + 1:]
    runpy.run_path(sys.argv[0], run_name="__main__")


if __name__ == "__main__":
    main()
