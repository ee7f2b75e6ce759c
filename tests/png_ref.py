"""A PNG reader for the tests of the library's writer (urt_host_write_png): the chunk walk with its CRCs and a zlib decode of
8-bit RGB rows with filter 0, which is all the writer emits.  Independent of any imaging library."""
import struct
import zlib

import numpy as np


def read_png(path):
    """(width, height, bit depth, colour type, (h, w, 3) uint8 pixels with the rows top-down as the file stores them)."""
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, {}
    while pos < len(data):
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + body)
        chunks[tag] = chunks.get(tag, b"") + body
        pos += 12 + n
    w, h, depth, ctype = struct.unpack(">IIBB", chunks[b"IHDR"][:10])
    assert (depth, ctype) == (8, 2)
    raw = np.frombuffer(zlib.decompress(chunks[b"IDAT"]), np.uint8).reshape(h, 1 + w * 3)
    assert (raw[:, 0] == 0).all()
    return w, h, depth, ctype, raw[:, 1:].reshape(h, w, 3)
