"""The implicit-GEMM Conv1d tile's dispatch rule restated (csrc/conv1d_tm.h conv_ksteps / conv_splits), for
the GPU tests that name the kernel variant each of their shapes takes."""


def splits(T_out, Cin, Cout, k, groups=1):
    """True = the 32-position kernel whose waves split K, False = the 128-position kernel.  Cin, Cout per
    group (or per phase of a transposed convolution, with groups = the phases and k its taps)."""
    steps = sum(-(-k * min(64, Cin - c0) // 32) for c0 in range(0, Cin, 64))
    return steps >= 4 and -(-T_out // 128) * -(-Cout // 64) * groups < 256
