"""Malformed input files of the command-line tools, shared by the tests that
hand them to the readers directly (test_cli_io.py, under the host sanitizers)
and through jxg_cjxl (test_cli_options.py): each must be refused with one
message, never read outside its buffer or sized before it is checked."""
import struct
import zlib

SIG = b"\x89PNG\r\n\x1a\n"
MAX_SIDE = 1 << 18  # jxg_cli::kMaxSide, jxg_encode_rgb8's limit


def chunk(t, d):
    return struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d) & 0xFFFFFFFF)


def ihdr(w, h, ctype=2):
    return struct.pack(">IIBBBBB", w, h, 8, ctype, 0, 0, 0)


def bad_pngs():
    """name -> bytes"""
    idat = chunk(b"IDAT", zlib.compress(b"\0" * 4))  # a 1 x 1 RGB image's rows
    out = {"ihdr_len%d" % n: SIG + chunk(b"IHDR", ihdr(1, 1)[:n]) for n in (0, 4, 12)}
    out["idat_before_ihdr"] = SIG + idat + chunk(b"IHDR", ihdr(1, 1)) + chunk(b"IEND", b"")
    out["no_idat"] = SIG + chunk(b"IHDR", ihdr(1, 1)) + chunk(b"IEND", b"")
    out["side_0"] = SIG + chunk(b"IHDR", ihdr(0, 1)) + idat + chunk(b"IEND", b"")
    out["side_over"] = SIG + chunk(b"IHDR", ihdr(MAX_SIDE + 1, 1)) + idat + chunk(b"IEND", b"")
    # the allocation bound: 2^18 x 2^18 RGB claimed over 60 bytes of IDAT
    stored = zlib.compress(bytes(49), 0)  # header 2 + stored block 5 + 49 + adler 4
    assert len(stored) == 60
    out["huge_over_60_bytes"] = (SIG + chunk(b"IHDR", ihdr(MAX_SIDE, MAX_SIDE))
                                 + chunk(b"IDAT", stored) + chunk(b"IEND", b""))
    return out


def bad_ppms():
    return {"side_over": b"P6 262145 1 255\n" + b"\0" * 64,
            "sides_u32_max": b"P6 4294967295 4294967295 255\n" + b"\0" * 64,
            "cut_short": b"P6 4 4 255\n" + b"\0" * 47}


def bad_pgms():
    return {"not_p5": b"P2\n2 2\n255\n" + b"\0" * 4,
            "maxval_254": b"P5\n2 2\n254\n" + b"\0" * 4,
            "wrong_data_size": b"P5\n2 2\n255\n" + b"\0" * 5}


def good_pgms():
    return {"comment_in_header": b"P5\n# a map\n2 2\n255\n" + b"\1\2\3\4"}
