"""A BGZF member parser written from the SAM specification, section 4.1 -- the judge of the BGZF tests.  Nothing here comes from the
library: the deflate streams are inflated by Python's zlib, the checksums are zlib.crc32.

A member is a gzip member (RFC 1952) with fixed fields ID1 = 31, ID2 = 139, CM = 8, FLG = 4 (FEXTRA), MTIME, XFL, OS, then XLEN and the
extra subfields, one of which is SI1 = 'B', SI2 = 'C', SLEN = 2 with BSIZE = total member size - 1; CDATA of BSIZE - XLEN - 19 bytes, a
raw deflate stream; CRC32 and ISIZE of the uncompressed data.  ISIZE is at most 65 536 by the specification."""
import struct
import zlib

BLOCK_IN = 65280          # the input bytes per block the writers of this project (and htslib) use
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


class BgzfError(ValueError):
    pass


def parse_member(buf, pos=0):
    """The member that starts at buf[pos]: (inflated bytes, member length, length of the deflate stream, first deflate byte's BTYPE).
    Raises BgzfError for anything the specification does not allow."""
    if len(buf) - pos < 28:
        raise BgzfError(f"member at {pos}: {len(buf) - pos} bytes left, the shortest member has 28")
    id1, id2, cm, flg, mtime, xfl, os_, xlen = struct.unpack_from("<BBBBIBBH", buf, pos)
    if (id1, id2, cm, flg) != (31, 139, 8, 4):
        raise BgzfError(f"member at {pos}: ID1 ID2 CM FLG = {id1} {id2} {cm} {flg}")
    if len(buf) - pos < 12 + xlen:
        raise BgzfError(f"member at {pos}: extra field cut short")
    bsize, x = None, pos + 12
    while x < pos + 12 + xlen:
        if pos + 12 + xlen - x < 4:
            raise BgzfError(f"member at {pos}: extra subfield cut short")
        si1, si2, slen = struct.unpack_from("<BBH", buf, x)
        if (si1, si2) == (66, 67):
            if slen != 2 or bsize is not None:
                raise BgzfError(f"member at {pos}: BC subfield with SLEN {slen} or given twice")
            bsize = struct.unpack_from("<H", buf, x + 4)[0]
        x += 4 + slen
    if x != pos + 12 + xlen or bsize is None:
        raise BgzfError(f"member at {pos}: extra subfields do not fill XLEN, or no BC subfield")
    total = bsize + 1
    if total > len(buf) - pos:
        raise BgzfError(f"member at {pos}: BSIZE + 1 = {total} but {len(buf) - pos} bytes left")
    n_cdata = bsize - xlen - 19
    if n_cdata < 1:
        raise BgzfError(f"member at {pos}: BSIZE {bsize} leaves no room for a deflate stream")
    cdata = bytes(buf[pos + 12 + xlen: pos + 12 + xlen + n_cdata])
    z = zlib.decompressobj(wbits=-15)
    try:
        data = z.decompress(cdata) + z.flush()
    except zlib.error as e:
        raise BgzfError(f"member at {pos}: inflate: {e}")
    if not z.eof:
        raise BgzfError(f"member at {pos}: the deflate stream does not end within CDATA")
    if z.unused_data:
        raise BgzfError(f"member at {pos}: {len(z.unused_data)} bytes of CDATA behind the end of the deflate stream")
    crc, isize = struct.unpack_from("<II", buf, pos + total - 8)
    if isize != len(data):
        raise BgzfError(f"member at {pos}: ISIZE {isize}, inflated {len(data)}")
    if crc != zlib.crc32(data):
        raise BgzfError(f"member at {pos}: CRC32 {crc:08x}, of the inflated bytes {zlib.crc32(data):08x}")
    if isize > 65536 or total > 65536:
        raise BgzfError(f"member at {pos}: ISIZE {isize} / size {total} above 65536")
    return data, total, n_cdata, (cdata[0] >> 1) & 3


def parse(buf):
    """Every member of buf, which must consist of whole members: a list of dicts (data, size, deflate_len, btype)."""
    out, pos = [], 0
    while pos < len(buf):
        data, total, n_cdata, btype = parse_member(buf, pos)
        out.append({"data": data, "size": total, "deflate_len": n_cdata, "btype": btype})
        pos += total
    return out


def inflate(buf):
    return b"".join(m["data"] for m in parse(buf))


def blocks_of(data):
    """data cut the way the writers cut it: every BLOCK_IN bytes, regardless of content."""
    return [data[i:i + BLOCK_IN] for i in range(0, len(data), BLOCK_IN)]


def zlib_deflate_len(block, level=1, strategy=zlib.Z_DEFAULT_STRATEGY):
    """Bytes of the raw deflate stream zlib makes of one block (the writers' parameters: wbits -15, memLevel 8)."""
    z = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    return len(z.compress(block) + z.flush())
