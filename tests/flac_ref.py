"""A small FLAC reference decoder and a small FLAC encoder in plain Python integers, for tests/test_flac*.py and tools/gen_golden_flac.py.
Written from the format description (include/dfx.h); no speed needed.  The decoder is strict: a CRC-8 or CRC-16 that does not
hold, a reserved code or a stream that ends early raises ``ValueError``.  The encoder writes what it is told — frame by frame, subframe by
subframe — so that every corner of the format can be put into a stream whose decoded samples are known: they are the encoder's input."""
from __future__ import annotations

import hashlib
from functools import lru_cache

import numpy as np


def _table(poly, bits):
    top, mask = 1 << (bits - 1), (1 << bits) - 1
    t = []
    for i in range(256):
        c = i << (bits - 8)
        for _ in range(8):
            c = ((c << 1) ^ poly) & mask if c & top else (c << 1) & mask
        t.append(c)
    return t


_T8, _T16 = _table(0x07, 8), _table(0x8005, 16)


def crc8(b) -> int:
    c = 0
    for x in b:
        c = _T8[c ^ x]
    return c


def crc16(b) -> int:
    c = 0
    for x in b:
        c = ((c << 8) & 0xFFFF) ^ _T16[(c >> 8) ^ x]
    return c


# ---------------------------------------------------------------------------------------------------------------- decoder
class BitReader:
    def __init__(self, data, at=0):
        self.d, self.p, self.acc, self.n = data, at, 0, 0

    def _byte(self):
        if self.p >= len(self.d):
            raise ValueError("stream ends inside a frame")
        self.acc = (self.acc << 8) | self.d[self.p]
        self.p += 1
        self.n += 8

    def read(self, k):
        while self.n < k:
            self._byte()
        self.n -= k
        v = self.acc >> self.n
        self.acc &= (1 << self.n) - 1
        return v

    def sread(self, k):
        v = self.read(k)
        return v - (1 << k) if k and v >> (k - 1) else v

    def unary(self):
        q = 0
        while True:
            if self.n == 0:
                self._byte()
            if self.acc == 0:
                q += self.n
                self.n = 0
                continue
            bl = self.acc.bit_length()
            q += self.n - bl
            self.n = bl - 1
            self.acc &= (1 << self.n) - 1
            return q

    def align(self):
        self.acc, self.n = 0, 0

    def tell(self):          # byte position when aligned
        return self.p - self.n // 8


def probe(data) -> dict:
    at = 0
    if data[:3] == b"ID3":
        size = (data[6] & 0x7F) << 21 | (data[7] & 0x7F) << 14 | (data[8] & 0x7F) << 7 | (data[9] & 0x7F)
        at = 10 + size + (10 if data[5] & 0x10 else 0)
    if data[at:at + 4] != b"fLaC":
        raise ValueError("no fLaC marker")
    at += 4
    info, last = None, False
    while not last:
        last, typ, size = bool(data[at] & 0x80), data[at] & 0x7F, int.from_bytes(data[at + 1:at + 4], "big")
        at += 4
        if typ == 0 and info is None:
            p = data[at:at + 34]
            w = int.from_bytes(p[10:18], "big")
            info = dict(min_block=int.from_bytes(p[0:2], "big"), max_block=int.from_bytes(p[2:4], "big"), sample_rate=w >> 44,
                        channels=((w >> 41) & 7) + 1, bps=((w >> 36) & 31) + 1, total=w & ((1 << 36) - 1), md5=bytes(p[18:34]))
        at += size
    if info is None:
        raise ValueError("no STREAMINFO")
    info["first_frame"] = at
    return info


FIXED = {0: [], 1: [1], 2: [2, -1], 3: [3, -3, 1], 4: [4, -6, 4, -1]}
_BPS_CODES = {1: 8, 2: 12, 4: 16, 5: 20, 6: 24}


def _residual(r, bs, order, out):
    method = r.read(2)
    if method > 1:
        raise ValueError("reserved residual method")
    pb, esc = (5, 31) if method else (4, 15)
    po = r.read(4)
    psize = bs >> po
    if psize << po != bs or psize < order:
        raise ValueError("bad partition order")
    for part in range(1 << po):
        cnt = psize - (order if part == 0 else 0)
        k = r.read(pb)
        if k == esc:
            w = r.read(5)
            out.extend(r.sread(w) if w else 0 for _ in range(cnt))
        else:
            for _ in range(cnt):
                u = (r.unary() << k) | r.read(k)
                out.append((u >> 1) ^ -(u & 1))


def _subframe(r, bs, bps):
    if r.read(1):
        raise ValueError("subframe padding bit")
    typ = r.read(6)
    wasted = r.unary() + 1 if r.read(1) else 0
    bps -= wasted
    if bps < 1:
        raise ValueError("wasted bits")
    if typ == 0:
        s = [r.sread(bps)] * bs
    elif typ == 1:
        s = [r.sread(bps) for _ in range(bs)]
    elif 8 <= typ <= 12 or typ >= 32:
        order = typ - 8 if typ < 32 else typ - 31
        if order > bs:
            raise ValueError("order above block size")
        s = [r.sread(bps) for _ in range(order)]
        if typ >= 32:
            prec = r.read(4) + 1
            if prec == 16:
                raise ValueError("reserved precision")
            shift = r.sread(5)
            if shift < 0:
                raise ValueError("negative shift")
            coefs = [r.sread(prec) for _ in range(order)]
        else:
            coefs, shift = FIXED[order], 0
        res = []
        _residual(r, bs, order, res)
        for x in res:
            n = len(s)
            s.append(x + (sum(c * s[n - 1 - j] for j, c in enumerate(coefs)) >> shift))
    else:
        raise ValueError("reserved subframe type")
    return [v << wasted for v in s] if wasted else s


def decode_frame(data, at, info) -> dict:
    """The frame that starts at byte ``at``: dict(bs, number, variable, end, chans [C][bs])."""
    r = BitReader(data, at)
    if r.read(14) != 0x3FFE or r.read(1):
        raise ValueError(f"no frame at byte {at}")
    variable = r.read(1)
    bsc, src, asg, ssc = r.read(4), r.read(4), r.read(4), r.read(3)
    if r.read(1) or bsc == 0 or src == 15 or asg > 10 or ssc in (3, 7):
        raise ValueError("reserved header code")
    b0 = r.read(8)
    num = b0
    if b0 & 0x80:
        ones = 0
        while b0 & (0x80 >> ones):
            ones += 1
        if ones < 2 or ones > 7:
            raise ValueError("bad coded number")
        num = b0 & (0x7F >> ones)
        for _ in range(ones - 1):
            c = r.read(8)
            if c & 0xC0 != 0x80:
                raise ValueError("bad coded number")
            num = (num << 6) | (c & 0x3F)
    bs = {1: 192}.get(bsc) or (576 << (bsc - 2) if 2 <= bsc <= 5 else (r.read(8) + 1 if bsc == 6 else (r.read(16) + 1 if bsc == 7 else 256 << (bsc - 8))))
    if src == 12:
        r.read(8)
    elif src in (13, 14):
        r.read(16)
    if crc8(data[at:r.tell()]) != r.read(8):
        raise ValueError(f"CRC-8 of the frame at byte {at}")
    bps = info["bps"] if ssc == 0 else _BPS_CODES[ssc]
    nch = asg + 1 if asg < 8 else 2
    side = {8: 1, 9: 0, 10: 1}.get(asg)
    ch = [_subframe(r, bs, bps + (1 if c == side else 0)) for c in range(nch)]
    if asg == 8:
        ch[1] = [a - b for a, b in zip(ch[0], ch[1])]
    elif asg == 9:
        ch[0] = [a + b for a, b in zip(ch[0], ch[1])]
    elif asg == 10:
        m = [(a << 1) | (b & 1) for a, b in zip(ch[0], ch[1])]
        ch = [[(a + b) >> 1 for a, b in zip(m, ch[1])], [(a - b) >> 1 for a, b in zip(m, ch[1])]]
    r.align()
    end = r.tell()
    if crc16(data[at:end]) != r.read(16):
        raise ValueError(f"CRC-16 of the frame at byte {at}")
    return dict(bs=bs, number=num, variable=variable, end=end + 2, chans=ch)


def decode(data):
    """-> (info, pcm int32 [C, T]); every frame from the first to the end of the data, each starting where the last one ended."""
    info = probe(data)
    at, chans = info["first_frame"], [[] for _ in range(info["channels"])]
    while at < len(data):
        fr = decode_frame(data, at, info)
        for c, s in zip(chans, fr["chans"]):
            c.extend(s)
        at = fr["end"]
    pcm = np.array(chans, dtype=np.int64)
    if info["total"]:
        pcm = pcm[:, :info["total"]]
    return info, pcm.astype(np.int32)


def md5_of(pcm, bps) -> bytes:
    """MD5 over the interleaved samples, little endian, ceil(bps / 8) bytes each."""
    nb = (bps + 7) // 8
    x = np.ascontiguousarray(np.asarray(pcm, np.int64).T).astype("<i8")
    return hashlib.md5(np.ascontiguousarray(x.view(np.uint8).reshape(-1, 8)[:, :nb]).tobytes()).digest()


# ---------------------------------------------------------------------------------------------------------------- encoder
class BitWriter:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def write(self, v, k):
        if k == 0:
            return
        assert 0 <= v < (1 << k), (v, k)
        self.acc = (self.acc << k) | v
        self.n += k
        while self.n >= 8:
            self.n -= 8
            self.out.append((self.acc >> self.n) & 0xFF)
        self.acc &= (1 << self.n) - 1

    def swrite(self, v, k):
        assert -(1 << (k - 1)) <= v < (1 << (k - 1)), (v, k)
        self.write(v & ((1 << k) - 1), k)

    def unary(self, q):
        while q >= 32:
            self.write(0, 32)
            q -= 32
        self.write(1, q + 1)

    def align(self):
        if self.n:
            self.write(0, 8 - self.n)


def _zigzag(r):
    return (r << 1) if r >= 0 else ((-r) << 1) - 1


def _best_k(us, kmax):
    return min(range(kmax + 1), key=lambda k: sum((u >> k) + 1 + k for u in us)) if us else 0


def lpc(signal, order, prec):
    """Least-squares predictor of ``order`` taps for ``signal``, quantised to ``prec`` bits: (coefs, shift)."""
    s = np.asarray(signal, np.float64)
    A = np.stack([s[order - 1 - j: len(s) - 1 - j] for j in range(order)], axis=1)
    c, *_ = np.linalg.lstsq(A + 1e-9 * np.random.default_rng(order).standard_normal(A.shape), s[order:], rcond=None)
    top = max(float(np.abs(c).max()), 1e-9)
    shift = max(0, min(15, prec - 2 - int(np.floor(np.log2(top))) - 1))
    q = np.clip(np.round(c * (1 << shift)), -(1 << (prec - 1)), (1 << (prec - 1)) - 1).astype(np.int64)
    return [int(v) for v in q], shift


def sub(kind, order=0, *, coefs=None, shift=0, prec=15, wasted=0, method=0, part_order=0, rice_k=None, escape=()):
    """A subframe's recipe.  kind: "const" | "verbatim" | "fixed" | "lpc" (coefs None: least squares at ``prec`` bits);
    rice_k: force that Rice parameter in every partition; escape: partitions written as raw samples (width 0 where all are zero)."""
    return dict(kind=kind, order=order, coefs=coefs, shift=shift, prec=prec, wasted=wasted, method=method, part_order=part_order, rice_k=rice_k,
                escape=tuple(escape))


def _write_subframe(w, s, bps, spec):
    bs, wasted, kind, order = len(s), spec["wasted"], spec["kind"], spec["order"]
    if wasted:
        assert all(v & ((1 << wasted) - 1) == 0 for v in s), "the low `wasted` bits must be zero"
        s = [v >> wasted for v in s]
        bps -= wasted
    typ = {"const": 0, "verbatim": 1, "fixed": 8 + order, "lpc": 31 + order}[kind]
    w.write(typ << 1 | (1 if wasted else 0), 8)
    if wasted:
        w.unary(wasted - 1)
    if kind == "const":
        assert all(v == s[0] for v in s)
        w.swrite(s[0], bps)
        return
    if kind == "verbatim":
        for v in s:
            w.swrite(v, bps)
        return
    for v in s[:order]:
        w.swrite(v, bps)
    if kind == "lpc":
        coefs, shift, prec = spec["coefs"], spec["shift"], spec["prec"]
        if coefs is None:
            coefs, shift = lpc(s, order, prec)
        assert len(coefs) == order
        w.write(prec - 1, 4)
        w.swrite(shift, 5)
        for c in coefs:
            w.swrite(c, prec)
    else:
        coefs, shift = FIXED[order], 0
    res = [s[n] - (sum(c * s[n - 1 - j] for j, c in enumerate(coefs)) >> shift) for n in range(order, bs)]
    assert all(-(1 << 31) <= r < (1 << 31) for r in res)
    method, po = spec["method"], spec["part_order"]
    pb, esc = (5, 31) if method else (4, 15)
    w.write(method, 2)
    w.write(po, 4)
    psize = bs >> po
    assert psize << po == bs and psize >= order
    at = 0
    for part in range(1 << po):
        cnt = psize - (order if part == 0 else 0)
        rs = res[at:at + cnt]
        at += cnt
        if part in spec["escape"]:
            width = 0 if all(r == 0 for r in rs) else max(max(r.bit_length() if r >= 0 else (-r - 1).bit_length() for r in rs) + 1, 1)
            w.write(esc, pb)
            w.write(width, 5)
            for r in rs:
                if width:
                    w.swrite(r, width)
            continue
        us = [_zigzag(r) for r in rs]
        k = spec["rice_k"] if spec["rice_k"] is not None else _best_k(us, esc - 1)
        w.write(k, pb)
        for u in us:
            w.unary(u >> k)
            w.write(u & ((1 << k) - 1), k)


_BS_CODES = {192: 1, 576: 2, 1152: 3, 2304: 4, 4608: 5, 256: 8, 512: 9, 1024: 10, 2048: 11, 4096: 12, 8192: 13, 16384: 14, 32768: 15}


def _utf8(v):
    if v < 0x80:
        return bytes([v])
    n = 2
    while v >= 1 << (5 * n + 1):
        n += 1
    out = [((0xFF << (8 - n)) & 0xFF) | (v >> (6 * (n - 1)))]
    out += [0x80 | ((v >> (6 * i)) & 0x3F) for i in range(n - 2, -1, -1)]
    return bytes(out)


def frame_header(bs, assign, bps, number, variable, explicit_bs=False, bps_code=None) -> bytes:
    code = None if explicit_bs else _BS_CODES.get(bs)
    tail = b""
    if code is None:
        code, tail = (6, bytes([bs - 1])) if bs <= 256 else (7, (bs - 1).to_bytes(2, "big"))
    ssc = {8: 1, 12: 2, 16: 4, 20: 5, 24: 6}.get(bps, 0) if bps_code is None else bps_code
    h = bytes([0xFF, 0xF8 | (1 if variable else 0), code << 4, (assign << 4) | (ssc << 1)]) + _utf8(number) + tail
    return h + bytes([crc8(h)])


def encode_frame(block, bps, assign, subs, number, variable=False, explicit_bs=False) -> bytes:
    """block: [C][bs] samples; the stereo modes 8 / 9 / 10 are formed here."""
    ch = [[int(v) for v in c] for c in block]
    bs = len(ch[0])
    if assign == 8:
        ch, bits = [ch[0], [a - b for a, b in zip(*ch)]], [bps, bps + 1]
    elif assign == 9:
        ch, bits = [[a - b for a, b in zip(*ch)], ch[1]], [bps + 1, bps]
    elif assign == 10:
        ch, bits = [[(a + b) >> 1 for a, b in zip(*ch)], [a - b for a, b in zip(*ch)]], [bps, bps + 1]
    else:
        assert assign == len(ch) - 1
        bits = [bps] * len(ch)
    w = BitWriter()
    for s, b, spec in zip(ch, bits, subs):
        _write_subframe(w, s, b, spec)
    w.align()
    body = frame_header(bs, assign, bps, number, variable, explicit_bs) + bytes(w.out)
    return body + crc16(body).to_bytes(2, "big")


def stream_head(bps, channels, total, min_block, max_block, sr=48000, md5=bytes(16), extra=b"", id3=False) -> bytes:
    word = (sr << 44) | ((channels - 1) << 41) | ((bps - 1) << 36) | total
    si = min_block.to_bytes(2, "big") + max_block.to_bytes(2, "big") + bytes(6) + word.to_bytes(8, "big") + md5
    blocks = bytes([0x00 if extra else 0x80]) + len(si).to_bytes(3, "big") + si
    if extra:   # a PADDING block behind STREAMINFO
        blocks += bytes([0x81]) + len(extra).to_bytes(3, "big") + extra
    tag = b"ID3\x04\x00\x00" + bytes([0, 0, 0, 7]) + b"\x00" * 7 if id3 else b""
    return tag + b"fLaC" + blocks


def encode(pcm, bps, frames, variable=False, sr=48000, with_md5=True, **head) -> bytes:
    """pcm [C, T] integers; frames: [(block size, channel assignment, [sub(...) per channel])], their block sizes summing to T."""
    pcm = np.asarray(pcm, np.int64)
    C, T = pcm.shape
    assert sum(f[0] for f in frames) == T
    first = frames[0][0]
    out, at = [], 0
    for i, (bs, assign, subs) in enumerate(frames):
        number = at if variable else i
        out.append(encode_frame(pcm[:, at:at + bs].tolist(), bps, assign, subs, number, variable, explicit_bs=(bs not in _BS_CODES)))
        at += bs
    sizes = [f[0] for f in frames]
    mn = min(sizes) if variable else first
    return stream_head(bps, C, T, mn, max(sizes), sr, md5_of(pcm, bps) if with_md5 else bytes(16), **head) + b"".join(out)


# ---------------------------------------------------------------------------------------------------------------- the case table
def _signal(rng, n, bps, amp=0.5):
    t = np.arange(n)
    x = np.sin(t * 0.031) + 0.5 * np.sin(t * 0.21 + 1.0) + 0.05 * rng.standard_normal(n)
    return np.clip(np.round(x / 1.6 * amp * (1 << (bps - 1))), -(1 << (bps - 1)), (1 << (bps - 1)) - 1).astype(np.int64)


@lru_cache(maxsize=1)
def cases() -> dict:
    """name -> (stream bytes, pcm int64 [C, T], bits per sample): every subframe kind, residual coding, stereo mode, wasted bits and bit depth
    the decoder has a path for, in streams of one to three short frames."""
    rng = np.random.default_rng(2024)
    out = {}

    def add(name, pcm, bps, frames, **kw):
        pcm = np.asarray(pcm, np.int64)
        out[name] = (encode(pcm, bps, frames, **kw), pcm, bps)

    mono = lambda n, bps=16, amp=0.5: _signal(rng, n, bps, amp)[None, :]   # noqa: E731
    add("const16", np.full((1, 16), -1234), 16, [(16, 0, [sub("const")])])
    add("verbatim192", rng.integers(-32768, 32768, (1, 192)), 16, [(192, 0, [sub("verbatim")])])
    for o in range(5):
        add(f"fixed{o}", mono(192 + 16), 16, [(192, 0, [sub("fixed", o)]), (16, 0, [sub("fixed", o)])])
    for o in (1, 8, 12, 32):
        add(f"lpc{o}", mono(1152), 16, [(1152, 0, [sub("lpc", o)])])
    add("blocks_fixed_strategy", mono(4096 + 4096 + 37), 16, [(4096, 0, [sub("lpc", 8, part_order=3)]), (4096, 0, [sub("fixed", 2, part_order=3)]),
                                                             (37, 0, [sub("fixed", 1)])])
    add("blocks_variable_strategy", mono(1152 + 16 + 4096), 16, [(1152, 0, [sub("fixed", 2)]), (16, 0, [sub("fixed", 1)]),
                                                               (4096, 0, [sub("lpc", 5, prec=12, part_order=3)])], variable=True)
    add("rice5", mono(192, 24, 0.9), 24, [(192, 0, [sub("fixed", 0, method=1)])])
    x = mono(192)
    x[0, 96:] = x[0, 95]                                      # the second partition of a fixed-1 residual is all zero: escape width 0
    add("escape", x, 16, [(192, 0, [sub("fixed", 1, part_order=1, escape=(0, 1))])])
    add("escape_rice5", mono(256), 16, [(256, 0, [sub("fixed", 2, method=1, part_order=2, escape=(1, 3))])])
    add("long_unary", rng.integers(-200, 200, (1, 192)), 16, [(192, 0, [sub("fixed", 0, rice_k=0)])])   # quotients up to ~400 zeros
    st = np.stack([_signal(rng, 1152, 16), _signal(rng, 1152, 16)])
    st[1] = st[0] // 2 + st[1] // 4 + 1                       # correlated, and odd mid/side sums among them
    for asg, nm in ((8, "left_side"), (9, "side_right"), (10, "mid_side")):
        add(nm, st, 16, [(1152, asg, [sub("lpc", 8), sub("fixed", 2)])])
    assert ((st[0] + st[1]) & 1).any()
    add("ch3", np.stack([_signal(rng, 192, 16) for _ in range(3)]), 16, [(192, 2, [sub("fixed", 2), sub("verbatim"), sub("lpc", 4)])])
    add("ch8", np.stack([_signal(rng, 192, 16) for _ in range(8)]), 16, [(192, 7, [sub("fixed", c % 5) for c in range(8)])] * 1)
    add("wasted1", mono(192, 16, 0.2) * 2, 16, [(192, 0, [sub("fixed", 2, wasted=1)])])
    add("wasted5", mono(192, 16, 0.02) * 32, 16, [(192, 0, [sub("lpc", 4, prec=10, wasted=5)])])
    add("wasted_stereo", np.stack([mono(192, 16, 0.1)[0] * 8, mono(192, 16, 0.1)[0] * 8]), 16, [(192, 10, [sub("fixed", 1, wasted=2), sub("fixed", 1, wasted=2)])])
    for bps in (8, 12, 20, 24):
        add(f"bps{bps}", np.stack([_signal(rng, 192, bps), _signal(rng, 192, bps)]), bps, [(192, 10, [sub("lpc", 6, prec=12), sub("fixed", 2)])])
    # full scale at 24 bits, 15-bit coefficients: the predictor's sum needs far more than 32 bits
    t = np.arange(1152)
    full = np.round(np.sin(t * 0.05) * ((1 << 23) - 1)).astype(np.int64)[None, :]
    add("wide24", full, 24, [(1152, 0, [sub("lpc", 8, prec=15)])])
    coefs, shift = lpc(full[0], 8, 15)
    assert max(abs(sum(c * int(full[0, n - 1 - j]) for j, c in enumerate(coefs))) for n in range(8, 1152)) > 1 << 33
    # a 16-bit side channel at +-65535 under a high-precision predictor
    l = np.where(np.arange(1152) // 3 % 2 == 0, 32767, -32768)
    add("side17", np.stack([l, -1 - l]), 16, [(1152, 8, [sub("fixed", 1), sub("lpc", 8, prec=15)])])
    assert (l - (-1 - l)).max() == 65535 and (l - (-1 - l)).min() == -65535
    # adversarial sync: 8-bit verbatim samples that spell a complete frame header with its CRC-8, byte-aligned inside the payload
    fake = frame_header(192, 0, 8, 1, False)
    body = rng.integers(-128, 128, 192)
    at = 192 - 64
    body[at:at + len(fake)] = [b - 256 if b >= 128 else b for b in fake]
    add("adversarial_sync", body[None, :], 8, [(192, 0, [sub("verbatim")])])
    blob = out["adversarial_sync"][0]
    assert blob.count(fake) == 1 and blob.index(fake) > probe(blob)["first_frame"] + 8
    add("id3_and_padding", mono(192), 16, [(192, 0, [sub("fixed", 2)])], extra=bytes(40), id3=True)
    return out
