"""csrc/np_sums.h and csrc/cube_means.h under the host's sanitizers: builds tests/np_sums_main.cpp (a program of its
own, AddressSanitizer and UndefinedBehaviorSanitizer linked statically, nothing of the library in it) and runs it as a
child process on the largest geometries of test_np_sums_host.py's sweep and on sums up to 100003 terms.  What it
watches: the frame stack of 40 in np_pairwise_sum, and the index arithmetic of BlockAt and RowAt on fields held in
buffers of exactly rows x cols values -- the padding must never be read.  It must exit clean.  No GPU."""
import np_sums_cases as K

SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]


def test_sums_and_block_means_under_sanitizers(tmp_path):
    exe = K.build(tmp_path, ["-O1", "-g", "-fno-omit-frame-pointer"] + SANITIZE)
    lengths = [0, 1, 7, 8, 9, 127, 128, 129, 1100, 4104, 8191, 8192, 8193, 16385, 100003]
    cases = [("sum", K.sum_values(n, 0)) for n in lengths]
    cases += [("mean", K.field(rows, cols, nan_share, 3), c) for rows, cols, c in K.LARGEST for nan_share in (0.0, 0.1)]
    assert all(g in K.GEOMETRIES for g in K.LARGEST)
    _, stdout = K.run(exe, tmp_path, cases)
    assert stdout.splitlines()[-2].startswith("%d sums, %d fields, " % (len(lengths), 2 * len(K.LARGEST))), stdout
