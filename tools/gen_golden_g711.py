#!/usr/bin/env python3
"""Writes tests/golden/g711_tables.npz: the G.711 codec as tables, from Python's `audioop` (3.12 and older).

    dec_ulaw, dec_alaw   int16 [256]     the 16-bit linear value of every code (audioop.ulaw2lin / alaw2lin)
    enc_ulaw, enc_alaw   uint8 [65536]   the code of every int16 value s, at index s + 32768: s >= 0 from audioop.lin2ulaw / lin2alaw;
                                         s < 0 by G.711's sign-magnitude rule, the code of -s with the sign bit flipped (s = -32768: of
                                         32767, the encoders clip below that) — audioop floors there (s >> 2) and differs in 381 (mu-law)
                                         and 127 (A-law) values, libsndfile and the library take the magnitude

    python tools/gen_golden_g711.py [--check]      # --check: compare with the committed file instead of writing it"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "golden", "g711_tables.npz")


def tables():
    import audioop

    codes = bytes(range(256))
    pos = np.arange(0, 32768, dtype="<i2").tobytes()
    out = {}
    for law, lin2, to_lin in (("ulaw", audioop.lin2ulaw, audioop.ulaw2lin), ("alaw", audioop.lin2alaw, audioop.alaw2lin)):
        out["dec_" + law] = np.frombuffer(to_lin(codes, 2), dtype="<i2").astype(np.int16)
        enc_pos = np.frombuffer(lin2(pos, 2), dtype=np.uint8)            # s = 0 .. 32767
        enc = np.empty(65536, np.uint8)
        enc[32768:] = enc_pos
        mag = np.minimum(np.arange(32768, 0, -1), 32767)                # |s| of s = -32768 .. -1, clipped
        enc[:32768] = enc_pos[mag] ^ 0x80
        out["enc_" + law] = enc
    return out


def main():
    t = tables()
    if "--check" in sys.argv:
        with np.load(OUT) as z:
            bad = [k for k in t if not np.array_equal(z[k], t[k])]
        print("differs: " + ", ".join(bad) if bad else "identical")
        return 1 if bad else 0
    np.savez_compressed(OUT, **t)
    print(OUT, os.path.getsize(OUT), "bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
