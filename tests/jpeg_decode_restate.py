"""numpy restatement of libjpeg-turbo's default decode of a baseline JPEG file -- the oracle of tests/test_jpegdec.py.

Scope: SOF0, 8 bit, one interleaved scan without restart markers, one component or YCbCr at 4:4:4 / 4:2:2 / 4:2:0.
`decode(file)` is the sequential decoder: Huffman decoding, jidctint's "islow" IDCT, jdsample's fancy up-sampling over the
real chroma samples with the edge replicated, jdcolor's fixed-point conversion; where PIL is built on libjpeg-turbo it equals
np.asarray(Image.open(f).convert("RGB")) pixel for pixel.  `simulate(file, S)` plays the self-synchronising rule of
csrc/jpegdec.hip on the same stream: subsequences of S bits, every lane decodes from a guessed state and then again from the
state its left neighbour ended in, until a pass changes no end state.  Integer arithmetic only."""
import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                   28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
                   54, 47, 55, 62, 63])      # natural index of the k-th coefficient of the scan


class Unsupported(ValueError):
    pass


def parse(data):
    """dict(H, W, ncomp, hs, vs, quant [ncomp][64] natural order, comp_dc, comp_ac, counts [4][16], vals [4][...], scan_off,
    scan_len) of a file in scope; raises Unsupported otherwise.  Tables 0...3 are DC 0, DC 1, AC 0, AC 1."""
    d = bytes(data)
    if len(d) < 4 or d[:2] != b"\xff\xd8":
        raise Unsupported("no SOI")
    qt, counts, vals, sof, p = {}, [None] * 4, [None] * 4, None, 2
    while True:
        if p + 4 > len(d):
            raise Unsupported("truncated header")
        if d[p] != 0xFF:
            raise Unsupported("no marker")
        m = d[p + 1]
        if m == 0xFF:
            p += 1
            continue
        if m == 0x01 or 0xD0 <= m <= 0xD8:
            p += 2
            continue
        n = d[p + 2] << 8 | d[p + 3]
        if n < 2 or p + 2 + n > len(d):
            raise Unsupported("truncated header")
        seg = d[p + 4:p + 2 + n]
        if m == 0xDB:
            o = 0
            while o < len(seg):
                if seg[o] >> 4:
                    raise Unsupported("16-bit DQT")
                t = np.zeros(64, dtype=np.int64)
                t[ZIGZAG] = list(seg[o + 1:o + 65])
                qt[seg[o] & 15] = t
                o += 65
        elif m == 0xC4:
            o = 0
            while o < len(seg):
                tc, th = seg[o] >> 4, seg[o] & 15
                if tc > 1 or th > 1:
                    raise Unsupported("Huffman table id")
                c = list(seg[o + 1:o + 17])
                counts[2 * tc + th], vals[2 * tc + th] = c, list(seg[o + 17:o + 17 + sum(c)])
                o += 17 + sum(c)
        elif m == 0xC0:
            if seg[0] != 8:
                raise Unsupported("precision")
            sof = dict(H=seg[1] << 8 | seg[2], W=seg[3] << 8 | seg[4], ncomp=seg[5],
                       comps=[(seg[6 + 3 * c], seg[7 + 3 * c] >> 4, seg[7 + 3 * c] & 15, seg[8 + 3 * c]) for c in range(seg[5])])
            if sof["ncomp"] not in (1, 3):
                raise Unsupported("components")
        elif 0xC1 <= m <= 0xCF:
            raise Unsupported("SOF%d" % (m - 0xC0))
        elif m == 0xDD:
            if seg[0] << 8 | seg[1]:
                raise Unsupported("restart interval")
        elif m == 0xDA:
            if sof is None or seg[0] != sof["ncomp"]:
                raise Unsupported("scan")
            break
        p += 2 + n
    nc = sof["ncomp"]
    hs, vs = (1, 1) if nc == 1 else sof["comps"][0][1:3]
    if nc == 3 and (any(c[1:3] != (1, 1) for c in sof["comps"][1:]) or (hs, vs) not in ((1, 1), (2, 1), (2, 2))):
        raise Unsupported("sampling")
    off = p + 2 + n
    e = off
    while e < len(d) and not (d[e] == 0xFF and e + 1 < len(d) and d[e + 1] != 0 and not 0xD0 <= d[e + 1] <= 0xD7):
        e += 1
    if e == len(d) and d[-1] == 0xFF:
        e -= 1
    return dict(H=sof["H"], W=sof["W"], ncomp=nc, hs=hs, vs=vs, quant=[qt[c[3]] for c in sof["comps"]],
                comp_dc=[seg[2 + 2 * c] >> 4 for c in range(nc)], comp_ac=[seg[2 + 2 * c] & 15 for c in range(nc)],
                counts=counts, vals=vals, scan_off=off, scan_len=e - off)


def unstuff(scan):
    """The scan without the 00 behind each FF; (bytes, number of stuffed bytes removed)."""
    a = np.frombuffer(bytes(scan), dtype=np.uint8)
    drop = np.zeros(a.size, dtype=bool)
    drop[1:] = (a[1:] == 0) & (a[:-1] == 0xFF)
    return a[~drop], int(drop.sum())


def _lut16(counts, vals):
    """16 leading bits -> (length, symbol), length 0 where no code matches: Annex C's canonical codes."""
    ln, sy = np.zeros(1 << 16, dtype=np.int64), np.zeros(1 << 16, dtype=np.int64)
    if counts is None:
        return ln.tolist(), sy.tolist(), 0
    code, k, longest = 0, 0, 0
    for l in range(1, 17):
        for _ in range(counts[l - 1]):
            ln[code << (16 - l):(code + 1) << (16 - l)] = l
            sy[code << (16 - l):(code + 1) << (16 - l)] = vals[k]
            code, k, longest = code + 1, k + 1, l
        code <<= 1
    return ln.tolist(), sy.tolist(), longest


class _Stream:
    """What both decoders share: the unstuffed scan as one 40-bit window per byte position, the tables, the MCU layout."""

    def __init__(self, data):
        info = self.info = parse(data)
        scan, self.stuffed = unstuff(bytes(data)[info["scan_off"]:info["scan_off"] + info["scan_len"]])
        self.nbits = 8 * scan.size
        pad = np.concatenate([scan, np.full(8, 0xFF, dtype=np.uint8)]).astype(np.uint64)
        w = np.zeros(scan.size + 4, dtype=np.uint64)
        for j in range(5):
            w = (w << np.uint64(8)) | pad[j:j + scan.size + 4]
        self.win = w.tolist()
        self.luts = [_lut16(info["counts"][t], info["vals"][t]) for t in range(4)]
        nc, hs, vs = info["ncomp"], info["hs"], info["vs"]
        self.bpm = 1 if nc == 1 else hs * vs + 2
        self.comp = [0] if nc == 1 else [0] * (hs * vs) + [1, 2]
        self.mx, self.my = -(-info["W"] // (8 * hs)), -(-info["H"] // (8 * vs))
        self.nblk = self.mx * self.my * self.bpm
        self.tdc = [info["comp_dc"][c] for c in self.comp]
        self.tac = [2 + info["comp_ac"][c] for c in self.comp]
        self.zrl, self.longest = 0, 0

    def run(self, pos, blk, k, limit, coef=None, gblk=0):
        """Decode from (pos, blk, k) until pos >= limit; a symbol that starts before the limit is finished.  A missing code
        consumes 16 bits and leaves the state.  Returns (pos, blk, k, blocks completed, position behind block nblk - 1 or -1)."""
        win, luts, tdc, tac, bpm, nblk, zz = self.win, self.luts, self.tdc, self.tac, self.bpm, self.nblk, ZIGZAG
        done, endpos = 0, -1
        while pos < limit:
            bits = (win[pos >> 3] >> (8 - (pos & 7))) & 0xFFFFFFFF
            ln, sy, _ = luts[tdc[blk] if k == 0 else tac[blk]]
            n = ln[bits >> 16]
            if n == 0:
                pos += 16
                continue
            sym = sy[bits >> 16]
            s = sym & 15
            v = 0
            if s:
                v = (bits >> (32 - n - s)) & ((1 << s) - 1)
                if v < 1 << (s - 1):
                    v -= (1 << s) - 1
            pos += n + s
            if coef is not None and n > self.longest:
                self.longest = n
            if k == 0:
                if coef is not None and gblk < nblk:
                    coef[gblk, 0] = v
                k = 1
            elif s == 0:
                if sym >> 4 == 15:
                    k += 16
                    self.zrl += coef is not None
                else:
                    k = 64
            else:
                k += sym >> 4
                if coef is not None and k < 64 and gblk < nblk:
                    coef[gblk, zz[k]] = v
                k += 1
            if k >= 64:
                k, blk, done, gblk = 0, (blk + 1) % bpm, done + 1, gblk + 1
                if gblk == nblk:
                    endpos = pos
        return pos, blk, k, done, endpos


def _idct(c):
    """jidctint.c on [n,8,8] int64 dequantised coefficients -> [n,8,8] samples 0...255."""
    def one(x, shift):      # along the last axis of [..., 8]
        i = [x[..., j] for j in range(8)]
        z1 = (i[2] + i[6]) * 4433
        t2, t3 = z1 - i[6] * 15137, z1 + i[2] * 6270
        t0, t1 = (i[0] + i[4]) << 13, (i[0] - i[4]) << 13
        t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
        t0, t1, t2, t3 = i[7], i[5], i[3], i[1]
        z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
        z5 = (z3 + z4) * 9633
        t0, t1, t2, t3 = t0 * 2446, t1 * 16819, t2 * 25172, t3 * 12299
        z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
        t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
        out = [t10 + t3, t11 + t2, t12 + t1, t13 + t0, t13 - t0, t12 - t1, t11 - t2, t10 - t3]
        return np.stack([(o + (1 << (shift - 1))) >> shift for o in out], axis=-1)
    w = one(c.transpose(0, 2, 1), 11).transpose(0, 2, 1)      # columns first
    return np.clip(one(w, 18) + 128, 0, 255)


def _h2v1(s):
    n = s.shape[1]
    i = np.arange(n)
    out = np.empty((s.shape[0], 2 * n), dtype=np.int64)
    out[:, 0::2] = (3 * s + s[:, np.maximum(i - 1, 0)] + 1) >> 2
    out[:, 1::2] = (3 * s + s[:, np.minimum(i + 1, n - 1)] + 2) >> 2
    return out


def _h2v2(s):
    ch, n = s.shape
    y, i = np.arange(ch), np.arange(n)
    out = np.empty((2 * ch, 2 * n), dtype=np.int64)
    for odd, far in ((0, s[np.maximum(y - 1, 0)]), (1, s[np.minimum(y + 1, ch - 1)])):
        r = 3 * s + far
        out[odd::2, 0::2] = (3 * r + r[:, np.maximum(i - 1, 0)] + 8) >> 4
        out[odd::2, 1::2] = (3 * r + r[:, np.minimum(i + 1, n - 1)] + 7) >> 4
    return out


def decode(data, stats=None):
    """uint8 [H,W,3] RGB of the file.  stats (a dict) receives what the stream exercises: scan_bits, stuffed, longest_code,
    zrl, blocks, end_bit."""
    st = _Stream(data)
    info = st.info
    coef = np.zeros((st.nblk, 64), dtype=np.int64)
    pos, blk, k, done, endpos = st.run(0, 0, 0, st.nbits, coef, 0)
    if done < st.nblk:
        raise ValueError("the scan holds %d of %d blocks" % (done, st.nblk))
    if stats is not None:
        stats.update(scan_bits=st.nbits, stuffed=st.stuffed, longest_code=st.longest, zrl=st.zrl, blocks=done, end_bit=endpos)
    H, W, nc, hs, vs = info["H"], info["W"], info["ncomp"], info["hs"], info["vs"]
    planes = []
    for c in range(nc):
        sel = np.array([r for r in range(st.bpm) if st.comp[r] == c])
        blocks = coef.reshape(st.mx * st.my, st.bpm, 64)[:, sel]          # [mcu, blocks of c, 64]
        blocks[:, :, 0] = np.cumsum(blocks[:, :, 0].reshape(-1)).reshape(blocks.shape[:2])      # DC prediction, scan order
        px = _idct((blocks * info["quant"][c]).reshape(-1, 8, 8))
        h, v = (hs, vs) if c == 0 and nc == 3 else (1, 1)
        px = px.reshape(st.my, st.mx, v, h, 8, 8).transpose(0, 2, 4, 1, 3, 5).reshape(st.my * v * 8, st.mx * h * 8)
        planes.append(px)
    Y = planes[0][:H, :W]
    if nc == 1:
        return np.repeat(Y[:, :, None], 3, axis=2).astype(np.uint8)
    ch, cw = -(-H // vs), -(-W // hs)
    up = []
    for p in planes[1:]:
        s = p[:ch, :cw]                                                   # the real samples only
        s = s if hs == 1 else (_h2v1(s) if vs == 1 else _h2v2(s))
        up.append(s[:H, :W] - 128)
    cb, cr = up
    R = Y + ((91881 * cr + 32768) >> 16)
    G = Y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    B = Y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([R, G, B], axis=2), 0, 255).astype(np.uint8)


def default_subseq_bits(scan_bytes):
    """The S the engine picks for scans of up to `scan_bytes` stuffed bytes: at most 1024 subsequences, at least 1024 bits."""
    per = -(-8 * scan_bytes // 1024)
    return max(1024, -(-per // 32) * 32)


def simulate(data, S):
    """(passes behind the first including the confirming one, blocks completed per subsequence at the fixed point, status) of the pass rule."""
    st = _Stream(data)
    n = -(-st.nbits // S)
    limit = [min((i + 1) * S, st.nbits) for i in range(n)]
    start = [(i * S, 0, 0) for i in range(n)]
    res = [st.run(i * S, 0, 0, limit[i]) for i in range(n)]
    end, cnt = [r[:3] for r in res], [r[3] for r in res]
    passes = 0                            # pass 0 is the guess; the passes behind it are counted, the confirming one included
    while True:
        prev, changed = list(end), False
        for i in range(1, n):
            if prev[i - 1] != start[i]:
                start[i] = prev[i - 1]
                r = st.run(*start[i], limit[i])
                changed |= r[:3] != end[i]
                end[i], cnt[i] = r[:3], r[3]
        passes += 1
        if not changed:
            break
    total, base, endpos = sum(cnt), 0, -1
    for i in range(n):                    # the emit step: where block nblk - 1 ends
        if base < st.nblk <= base + cnt[i]:
            endpos = st.run(*start[i], limit[i], None, base)[4]
        base += cnt[i]
    status = 1 if total < st.nblk else 2 if total > st.nblk else 0 if st.nbits - 8 < endpos <= st.nbits else 3
    return passes, cnt, status
