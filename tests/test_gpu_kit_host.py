"""CPU tier: the host branch of the padded call (tests/gpu_kit.py) against entry points made here with ctypes.CFUNCTYPE — no library, no
device.  What the GPU tests rely on: an output written exactly is seen as untouched, a word too many or a word before the list is
seen, a short list is judged by its own length, what was not asked for arrives as a null pointer, and the fills are the documented ones."""
import ctypes as C

import numpy as np

from tests.gpu_kit import BYTE_FILL, WORD_FILL, Padded, PaddedCall, at

PAD = 3
WORDS = 16                   # 32-bit words of a record


def _no_device(*args):
    raise AssertionError("the host branch called the device twin")


def _writer(count, value=7):
    """fake entry point: `count` words of `value` from the pointer on"""
    @C.CFUNCTYPE(C.c_int, C.c_void_p)
    def fn(p):
        C.cast(p, C.POINTER(C.c_uint32 * max(count, 1)))[0][:count] = [value] * count
        return 0
    return fn


def test_exactly_n_items_written_and_one_too_many():
    n = 5
    out = Padded(n, back=PAD)
    assert PaddedCall(host=True)(_writer(n), _no_device, out) == 0
    assert np.array_equal(out.body, np.full(n, 7, np.uint32)) and out.untouched() and (out.tail == WORD_FILL).all() and out.tail.size == PAD
    out = Padded(n, back=PAD)
    PaddedCall(host=True)(_writer(n + 1), _no_device, out)
    assert not out.untouched()


def test_the_front_pad_of_a_record_list_written():
    recs = Padded(4, words=WORDS, front=PAD, back=PAD)

    @C.CFUNCTYPE(C.c_int, C.c_void_p)
    def one_word_before(p):
        C.cast(p - 4, C.POINTER(C.c_uint32))[0] = 7
        return 0
    PaddedCall(host=True)(one_word_before, _no_device, recs)
    assert not recs.untouched() and not recs.untouched(written=0)
    assert not Padded.over(recs.a, words=WORDS, front=PAD).untouched(0)          # the same through the layout laid over the buffer


def test_fewer_records_than_the_capacity():
    cap, k = 6, 2
    recs = Padded(cap, words=WORDS, front=PAD, back=PAD)
    PaddedCall(host=True)(_writer(k * WORDS), _no_device, recs)
    assert recs.untouched(written=k) and not recs.untouched(written=k - 1) and not recs.untouched(written=0)
    assert recs.untouched() and recs.untouched(written=cap)                       # (judged as a full list: the pads alone)
    assert Padded.over(recs.a, words=WORDS, front=PAD).untouched(k) and not Padded.over(recs.a, words=WORDS, front=PAD).untouched(k - 1)


def test_what_was_not_asked_for_and_an_empty_input_are_null_pointers():
    seen = []

    @C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p)
    def fn(inp, n, hops, out, cnt):
        seen.append((inp, n, hops, out, cnt))
        return 3
    out, cnt = Padded(2, back=PAD), Padded(4)
    assert PaddedCall(host=True)(fn, _no_device, np.zeros((0, 3), np.float32), 0, None, None, cnt) == 3
    assert seen[-1] == (None, 0, None, None, cnt.a.ctypes.data)
    pts = np.zeros((2, 3), np.float32)
    PaddedCall(host=True)(fn, _no_device, pts, 2, None, out, cnt)
    assert seen[-1] == (pts.ctypes.data, 2, None, out.a.ctypes.data, cnt.a.ctypes.data)
    assert out.untouched() and cnt.untouched()


def test_the_fills_of_bytes_words_and_a_files_own():
    b, w, own = Padded(3, np.uint8, back=2), Padded(3, back=2), Padded(3, back=2, fill=0xDEADBEEF)
    assert b.a.dtype == np.uint8 and b.a.size == 5 and (b.a == 0x5A).all() and BYTE_FILL == 0x5A
    assert w.a.dtype == np.uint32 and w.a.size == 5 and (w.a == 0x5A5A5A5A).all() and WORD_FILL == 0x5A5A5A5A
    assert (own.a == 0xDEADBEEF).all() and own.untouched(0)
    own.a[4] = WORD_FILL
    assert not own.untouched()


def test_the_byte_offset_lands_on_the_first_record():
    recs = Padded(2, words=WORDS, front=PAD, back=PAD)
    assert recs.offset == PAD * WORDS * 4
    PaddedCall(host=True)(_writer(WORDS, 9), _no_device, recs)
    assert (recs.a.reshape(-1, WORDS)[PAD] == 9).all() and (recs.body[:WORDS] == 9).all() and recs.untouched(1) and not recs.untouched(0)
    # at(): bytes into an input — the six words in the middle of a wider record, and one byte further
    wide = np.arange(10, dtype=np.int32)
    seen = []

    @C.CFUNCTYPE(C.c_int, C.c_void_p)
    def fn(p):
        seen.append(p)
        return 0
    PaddedCall(host=True)(fn, _no_device, at(wide, 8))
    PaddedCall(host=True)(fn, _no_device, at(wide, 9))
    PaddedCall(host=True)(fn, _no_device, at(recs, 4))
    assert seen == [wide.ctypes.data + 8, wide.ctypes.data + 9, recs.a.ctypes.data + recs.offset + 4]
