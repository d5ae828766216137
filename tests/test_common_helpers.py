"""The shared helpers of tests/common.py are the strict ones: no GPU, no library, milliseconds.  What every `assert same_bits(a, b)` of the
suite means is pinned here, beside the round trip of the host programs and the refusal check."""
import os

import numpy as np
import pytest

from common import bits, halves, refused, run_host, same_bits

f32 = np.float32


def _nan(payload):
    return np.array([0x7FC00000 | payload], np.uint32).view(f32)


def test_same_bits_is_false_for_everything_but_the_same_bytes_of_the_same_kind():
    assert not same_bits(f32(0.0), f32(-0.0)) and f32(0.0) == f32(-0.0)
    assert not same_bits(_nan(1), _nan(2))
    a = np.linspace(-1.0, 1.0, 6).astype(f32)
    assert not same_bits(a, a.astype(np.float64)) and np.array_equal(a, a.astype(np.float64))
    assert not same_bits(a.reshape(2, 3), a)
    big = np.random.default_rng(0).standard_normal(1000).astype(f32)
    flipped = big.copy()
    flipped.view(np.uint32)[617] ^= 1
    assert not same_bits(big, flipped) and np.allclose(big, flipped, rtol=2e-7, atol=0.0)
    assert same_bits(big, big.copy()) and same_bits(_nan(5), _nan(5))


def test_same_bits_reads_a_view_in_its_own_order():
    m = np.arange(24, dtype=f32).reshape(4, 6)
    for view in (m[:, ::2], m.T, m[::-1]):
        assert not view.flags["C_CONTIGUOUS"] and same_bits(view, np.ascontiguousarray(view))
    assert not same_bits(m.T, m.reshape(6, 4))                               # the same bytes in memory, another array


def test_nan_equal_differs_from_the_strict_form_on_nan_against_nan_only():
    a = np.array([1.0, -0.0, np.inf, 3.5], f32)
    cases = [(f32(0.0), f32(-0.0)), (a, a.astype(np.float64)), (a.reshape(2, 2), a), (a, a + f32(1e-7) * a), (a, a.copy()),
             (np.arange(4, dtype=np.int32), np.arange(4, dtype=np.int32)), (np.arange(4, dtype=np.int32), np.arange(1, 5, dtype=np.int32))]
    for x, y in cases:
        assert same_bits(x, y, nan_equal=True) == same_bits(x, y)
    x, y = np.concatenate([a, _nan(1)]), np.concatenate([a, -_nan(2)])
    assert same_bits(x, y, nan_equal=True) and not same_bits(x, y)
    y[1] = 0.0                                                               # a NaN pair beside it hides nothing: - 0 against + 0
    assert not same_bits(x, y, nan_equal=True)
    assert not same_bits(_nan(1), f32([1.0]), nan_equal=True)                # a NaN against a number


def test_bits_round_trips_and_refuses_what_is_not_float32():
    a = np.array([[0.0, -0.0, 1.0], [np.inf, np.nan, 1e-45]], f32)
    b = bits(a)
    assert b.dtype == np.uint32 and b.shape == a.shape and b[0, 1] == 0x80000000 and b[0, 2] == 0x3F800000
    assert same_bits(b.view(f32), a)
    with pytest.raises(AssertionError):
        bits(a.astype(np.float64))


def test_halves_are_the_high_and_the_low_word():
    hi, lo = halves(np.array([0x0000000500000007, 0xFFFFFFFF00000000], np.uint64))
    assert hi.dtype == lo.dtype == np.int64 and hi.tolist() == [5, 0xFFFFFFFF] and lo.tolist() == [7, 0]


def _program(tmp_path, extra):
    """a stand-in for a host program: out.bin = in.bin (+ extra bytes)"""
    exe = tmp_path / "echo_host"
    exe.write_text('#!/bin/sh\ncat "$1" > "$2"\nprintf "%s" >> "$2"\n' % extra)
    os.chmod(exe, 0o755)
    return str(exe)


def test_run_host_consumes_every_output_byte(tmp_path):
    a = np.arange(5, dtype=f32)
    head, got = run_host(_program(tmp_path, ""), [], np.int32(5).tobytes(), [a], [(np.int32, 1), (f32, 5)])
    assert head.tolist() == [5] and same_bits(got, a)
    with pytest.raises(AssertionError):                                      # one byte more than the declared outputs
        run_host(_program(tmp_path, "x"), [], np.int32(5).tobytes(), [a], [(np.int32, 1), (f32, 5)])


def _raises(code, text="gs_bin: gs_preprocess first"):
    from gaussiansplat_amd import backend as B                              # (the module alone: no library is loaded)

    def call():
        raise B.GsError(code, text)
    return call


def test_refused_checks_the_code_the_text_and_that_the_call_raised():
    refused(_raises(-1))
    refused(_raises(-1), "gs_preprocess first")
    refused(_raises(-5), "gs_preprocess first", -5)
    with pytest.raises(AssertionError):                                      # the wrong code
        refused(_raises(-5))
    with pytest.raises(AssertionError):
        refused(_raises(-1), code=-5)
    with pytest.raises(AssertionError):                                      # the right code, the wrong text
        refused(_raises(-1), "gs_forward first")
    with pytest.raises(pytest.fail.Exception):                               # the call does not raise
        refused(lambda: None)
