"""Pure numpy restatement of the baseline grey JPEG encoder of csrc/jpegenc.hip -- libjpeg's encoder for one 8-bit
component, restated: integer "islow" FDCT (jfdctint), its quantiser rounding, jpeg_quality_scaling on the Annex K
luminance table, the Annex K luminance Huffman tables, 1-bit padding, FF -> FF 00 stuffing and the header libjpeg's JFIF
writer emits.  It is the oracle of tests/test_jpegenc.py on any machine; where PIL is built on libjpeg-turbo the test also
pins it to PIL.Image.save(format="JPEG", quality=q), byte for byte."""
import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                   28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
                   54, 47, 55, 62, 63])
BASE_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22,
                      29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103,
                      121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
DC_BITS = [0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]
DC_VALS = list(range(12))
AC_BITS = [0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D]
AC_VALS = [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32,
           0x81, 0x91, 0xA1, 0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16,
           0x17, 0x18, 0x19, 0x1A, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45,
           0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
           0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94,
           0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6,
           0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8,
           0xD9, 0xDA, 0xE1, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8,
           0xF9, 0xFA]
HEADER_LEN = 328


def quant_table(quality):
    """jpeg_quality_scaling + jpeg_add_quant_table(force_baseline): 64 values, natural order."""
    if not 1 <= quality <= 100:
        raise ValueError("quality outside 1..100")
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.clip((BASE_LUMA * scale + 50) // 100, 1, 255)


def _huff(bits, vals):
    """Symbol -> (code, length) by the canonical assignment of Annex C."""
    tab, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            tab[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return tab


DC_TAB, AC_TAB = _huff(DC_BITS, DC_VALS), _huff(AC_BITS, AC_VALS)


def header(H, W, quality):
    """SOI, APP0 (JFIF 1.01, units 0, density 1x1), DQT, SOF0, DHT (DC), DHT (AC), SOS: 328 bytes."""
    q = quant_table(quality)
    b = bytearray(b"\xff\xd8\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    b += b"\xff\xdb\x00\x43\x00" + bytes(int(v) for v in q[ZIGZAG])
    b += b"\xff\xc0\x00\x0b\x08" + bytes([H >> 8, H & 255, W >> 8, W & 255]) + b"\x01\x01\x11\x00"
    b += b"\xff\xc4\x00\x1f\x00" + bytes(DC_BITS) + bytes(DC_VALS)
    b += b"\xff\xc4\x00\xb5\x10" + bytes(AC_BITS) + bytes(AC_VALS)
    b += b"\xff\xda\x00\x08\x01\x01\x00\x00\x3f\x00"
    assert len(b) == HEADER_LEN
    return bytes(b)


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_pass(d, first):
    """One jfdctint pass along the last axis of d [..., 8] (int64)."""
    t0, t7, t1, t6 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7], d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5, t3, t4 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5], d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if first else 15
    out = np.empty_like(d)
    if first:
        out[..., 0], out[..., 4] = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        out[..., 0], out[..., 4] = _descale(t10 + t11, 2), _descale(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    out[..., 2] = _descale(z1 + t13 * 6270, n)
    out[..., 6] = _descale(z1 - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    out[..., 7] = _descale(t4 + z1 + z3, n)
    out[..., 5] = _descale(t5 + z2 + z4, n)
    out[..., 3] = _descale(t6 + z2 + z3, n)
    out[..., 1] = _descale(t7 + z1 + z4, n)
    return out


def quantised_blocks(img, quality):
    """[H, W] uint8 -> [nblk, 64] quantised coefficients in zigzag order, blocks in raster order."""
    img = np.asarray(img, dtype=np.uint8)
    H, W = img.shape
    Hp, Wp = (H + 7) // 8 * 8, (W + 7) // 8 * 8
    p = np.pad(img, ((0, Hp - H), (0, Wp - W)), mode="edge").astype(np.int64) - 128
    blk = p.reshape(Hp // 8, 8, Wp // 8, 8).transpose(0, 2, 1, 3).reshape(-1, 8, 8)
    c = _fdct_pass(blk, True)                                                  # rows
    c = _fdct_pass(c.transpose(0, 2, 1), False).transpose(0, 2, 1)             # columns
    div = (quant_table(quality) * 8).reshape(8, 8)
    qc = np.sign(c) * ((np.abs(c) + (div >> 1)) // div)
    return qc.reshape(-1, 64)[:, ZIGZAG]


def _value_bits(v):
    n = int(abs(v)).bit_length()
    return (v if v >= 0 else v - 1) & ((1 << n) - 1), n


def encode(img, quality=95, stats=None):
    """The JPEG file (bytes) of a grey map.  stats: a dict that receives scan_bits, scan_bytes (before stuffing), stuffed,
    zrl, max_dc_size and max_ac_size."""
    H, W = np.asarray(img).shape
    codes, lens = [], []
    last_dc = zrl = max_dc = max_ac = 0
    for zz in quantised_blocks(img, quality).tolist():
        v, n = _value_bits(zz[0] - last_dc)
        last_dc = zz[0]
        max_dc = max(max_dc, n)
        c, l = DC_TAB[n]
        codes.append((c << n) | v)
        lens.append(l + n)
        r = 0
        for k in range(1, 64):
            if zz[k] == 0:
                r += 1
                continue
            while r > 15:
                codes.append(AC_TAB[0xF0][0])
                lens.append(AC_TAB[0xF0][1])
                zrl += 1
                r -= 16
            v, n = _value_bits(zz[k])
            max_ac = max(max_ac, n)
            c, l = AC_TAB[(r << 4) | n]
            codes.append((c << n) | v)
            lens.append(l + n)
            r = 0
        if r > 0:
            codes.append(AC_TAB[0][0])
            lens.append(AC_TAB[0][1])
    codes, lens = np.array(codes, dtype=np.int64), np.array(lens, dtype=np.int64)
    total = int(lens.sum())
    start = np.repeat(np.cumsum(lens) - lens, lens)
    pos = np.arange(total) - start
    bits = (np.repeat(codes, lens) >> (np.repeat(lens, lens) - 1 - pos)) & 1
    bits = np.concatenate([bits, np.ones(-total % 8, dtype=np.int64)]).astype(np.uint8)
    scan = np.packbits(bits)
    ff = np.flatnonzero(scan == 255)
    stuffed = np.insert(scan, ff + 1, 0)
    if stats is not None:
        stats.update(scan_bits=total, scan_bytes=int(scan.size), stuffed=int(ff.size), zrl=zrl, max_dc_size=max_dc,
                     max_ac_size=max_ac)
    return header(H, W, quality) + stuffed.tobytes() + b"\xff\xd9"


def bound(H, W):
    """Worst-case file size: 20 + 63 * 26 bits per block, every scan byte stuffed, header and EOI."""
    nblk = ((H + 7) // 8) * ((W + 7) // 8)
    return HEADER_LEN + 2 * ((nblk * (20 + 63 * 26) + 7) // 8) + 2
