#!/usr/bin/env python3
"""tests/golden/flac_noise_mono.flac and flac_noise_stereo24f.flac: two real-encoder FLAC streams cut out of the reference's test data,
``assets/noise_flac.hdf5`` (an HDF5 file whose datasets are whole .flac files, stored as bytes).  Data only: the bytes are copied, nothing is
decoded or re-encoded here.

* mono: the stream from byte 3 649 818 to the end of the file (224 035 bytes): 48 kHz, 16 bits, 1 channel, 236 983 samples in 58 frames,
  STREAMINFO MD5 b9766d53a451a4b6a2b7283163e1bcff.
* stereo24f: the stream at byte 6144 (48 kHz, 16 bits, 2 independent channels): its metadata and its first 24 frames of 4096 samples, with
  STREAMINFO rewritten to 98 304 total samples and an all-zero MD5 ("not computed").  The frames are found by walking the chain with the
  reference decoder of tests/flac_ref.py (every CRC-8 and CRC-16 checked).
"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
OUT = os.path.join(REPO, "tests", "golden")
MONO_AT, STEREO_AT, STEREO_FRAMES = 3649818, 6144, 24


def main():
    from tests import flac_ref as R
    from tools.ref_import import REFERENCE_ROOT

    SRC = os.path.join(REFERENCE_ROOT, "assets", "noise_flac.hdf5")
    with open(SRC, "rb") as f:
        raw = f.read()
    mono = raw[MONO_AT:]
    assert mono[:4] == b"fLaC" and len(mono) == 224035
    with open(os.path.join(OUT, "flac_noise_mono.flac"), "wb") as f:
        f.write(mono)
    st = raw[STEREO_AT:]
    info = R.probe(st)
    assert (info["channels"], info["bps"], info["sample_rate"]) == (2, 16, 48000)
    at, total = info["first_frame"], 0
    for _ in range(STEREO_FRAMES):
        fr = R.decode_frame(st, at, info)
        at, total = fr["end"], total + fr["bs"]
    head = bytearray(st[:info["first_frame"]])
    si = head.index(b"fLaC") + 8                       # STREAMINFO body
    word = int.from_bytes(head[si + 10: si + 18], "big")
    word = (word >> 36 << 36) | total
    head[si + 10: si + 18] = word.to_bytes(8, "big")
    head[si + 18: si + 34] = bytes(16)
    with open(os.path.join(OUT, "flac_noise_stereo24f.flac"), "wb") as f:
        f.write(bytes(head) + st[info["first_frame"]: at])
    print("mono", len(mono), "stereo", len(head) + at - info["first_frame"], "samples", total)


if __name__ == "__main__":
    main()
