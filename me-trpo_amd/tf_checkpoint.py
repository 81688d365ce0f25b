"""TensorFlow 1.x checkpoints (tensor bundle V2, what tf.train.Saver.save writes) read and written with NumPy alone.

A checkpoint `<prefix>` is two files plus the directory's state file:

    <prefix>.index                    a LevelDB-format table: key "" -> BundleHeaderProto, key <variable name> -> BundleEntryProto
    <prefix>.data-00000-of-00001      the tensors' raw little-endian bytes, one after another
    checkpoint                        text CheckpointState: model_checkpoint_path: "<prefix>"   (Saver.save, latest_checkpoint)

Status: format-spec-pinned, reference-unpinned.  TensorFlow is not a dependency, and no checkpoint written by the reference
run ships with it, so every fact below is taken from the TF 1.x sources named next to it and is pinned here by tests written
from that specification (tests/test_tf_checkpoint.py), not by a file TF itself wrote.

core/lib/io/format.{h,cc}
  - Footer: the last 48 bytes.  metaindex BlockHandle, index BlockHandle (each varint64 offset, varint64 size), zero-padded
    to 40 bytes (2 x BlockHandle::kMaxEncodedLength), then the fixed64 magic 0xdb4775248b80fb57 (kTableMagicNumber).
  - Every block is followed by a 5-byte trailer (kBlockTrailerSize): a type byte (0 kNoCompression, 1 kSnappyCompression)
    and a fixed32 masked crc32c of the block contents AND the type byte.  A BlockHandle's size excludes the trailer.
core/lib/io/block_builder.cc, block.cc
  - Entries: varint32 shared, varint32 non_shared, varint32 value_length, key[shared:] (non_shared bytes), value.
    After the entries: fixed32 restart offsets, then a fixed32 restart count.  A restart entry has shared = 0.
core/lib/io/table_builder.cc, table_options.h
  - Data blocks are cut once they reach Options::block_size (default 262144) bytes; restart interval 16
    (block_restart_interval).  The index block holds one entry per data block (restart interval 1): a separator key
    >= every key of the block and < every key of the next, value = the block's BlockHandle.  The metaindex block is empty.
  - Keys are in bytewise order; a key is added once.
core/lib/hash/crc32c.h
  - crc32c is the Castagnoli CRC (reflected polynomial 0x82f63b78).  Mask(c) = ((c >> 15) | (c << 17)) + 0xa282ead8 mod 2^32
    (kMaskDelta), Unmask its inverse.
core/util/tensor_bundle/tensor_bundle.{h,cc,proto}
  - Header key is "" (kHeaderEntryKey).  BundleHeaderProto: num_shards = 1 (int32), endianness = 2 (enum, LITTLE 0, BIG 1),
    version = 3 (VersionDef: producer = 1 int32; kTensorBundleVersion = 1).
  - BundleEntryProto: dtype = 1 (enum DataType), shape = 2 (TensorShapeProto: repeated dim = 2, Dim.size = 1 int64),
    shard_id = 3 (int32), offset = 4 (int64), size = 5 (int64), crc32c = 6 (fixed32: the masked crc32c of the tensor's bytes),
    slices = 7 (repeated TensorSliceProto: present only for partitioned variables).
  - Data file of shard i of n: <prefix>.data-%05d-of-%05d.  BundleWriter writes no compression in the index.
core/framework/types.proto
  - DT_FLOAT 1, DT_DOUBLE 2, DT_INT32 3, DT_INT64 9 (the only dtypes this module reads or writes).
python/training/saver.py, checkpoint_state.proto
  - The state file `checkpoint` in the checkpoint's directory holds model_checkpoint_path = 1 and all_model_checkpoint_paths
    = 2 as a text proto; the paths may be relative to that directory.

Out of scope, each refused with CheckpointFormatError: V1 checkpoints, .meta graphs, sharded bundles, sliced variables,
big-endian bundles, other dtypes, snappy-compressed blocks.  Protobuf wire format is decoded by hand (no generated modules)."""
import os
import re
from collections import OrderedDict

import numpy as np

TABLE_MAGIC = 0xdb4775248b80fb57
FOOTER_LEN = 48
BLOCK_TRAILER = 5
MASK_DELTA = 0xa282ead8
DTYPES = {1: np.dtype('<f4'), 2: np.dtype('<f8'), 3: np.dtype('<i4'), 9: np.dtype('<i8')}
DTYPE_IDS = {np.dtype('float32'): 1, np.dtype('float64'): 2, np.dtype('int32'): 3, np.dtype('int64'): 9}
STATE_FILE = 'checkpoint'


class CheckpointFormatError(ValueError):
    """A file that is not a checkpoint this module reads; the message names the file and the check that failed."""

    def __init__(self, path, reason):
        self.path, self.reason = path, reason
        super(CheckpointFormatError, self).__init__('%s: %s' % (path, reason))


# ---------------------------------------------------------------------------------------------------------- crc32c
def _make_table():
    t = np.arange(256, dtype=np.uint32)
    for _ in range(8):
        t = np.where(t & 1, (t >> 1) ^ np.uint32(0x82f63b78), t >> 1).astype(np.uint32)
    return t


_TABLE = _make_table()
_TABLE_L = [int(x) for x in _TABLE]
_CHUNK = 4096


def _crc_bytes(reg, data):
    """Raw register update (no pre / post inversion), one byte at a time."""
    T = _TABLE_L
    for b in data:
        reg = T[(reg ^ b) & 0xff] ^ (reg >> 8)
    return reg


def crc32c_bytewise(data, crc=0):
    """Reference implementation: the standard table-driven loop.  `crc` continues an earlier value."""
    return _crc_bytes(crc ^ 0xffffffff, bytes(data)) ^ 0xffffffff


def _gf2_times(mat, vec):
    s, i = 0, 0
    while vec:
        if vec & 1:
            s ^= mat[i]
        vec >>= 1; i += 1
    return s


def _zeros_operator(nbytes):
    """32x32 GF(2) matrix (as 32 column words) that advances a raw register over `nbytes` zero bytes (zlib's crc32_combine)."""
    odd = [0x82f63b78] + [1 << i for i in range(31)]                # one zero bit
    even = [_gf2_times(odd, odd[i]) for i in range(32)]             # two zero bits
    odd = [_gf2_times(even, even[i]) for i in range(32)]            # four zero bits
    result = [1 << i for i in range(32)]                            # identity
    n, cur = nbytes, odd
    while True:                                                     # cur: operator for 8 * 2^j zero bits, squared each round
        cur = [_gf2_times(cur, cur[i]) for i in range(32)]
        if n & 1:
            result = [_gf2_times(cur, result[i]) for i in range(32)]
        n >>= 1
        if not n:
            return result


def _byte_tables(mat):
    """The operator as four 256-entry tables, one per byte of the register."""
    return [[_gf2_times(mat, v << (8 * k)) for v in range(256)] for k in range(4)]


_SHIFT_CHUNK = _byte_tables(_zeros_operator(_CHUNK))


def crc32c(data, crc=0):
    """crc32c of a bytes-like object.  Whole 4 KiB chunks are run side by side in NumPy (one byte of every chunk per step,
    from a zero register), then folded in order: reg <- shift_4096(reg) ^ chunk_crc, which holds because the raw register
    update is linear over GF(2).  The tail runs byte by byte.  Equal to crc32c_bytewise."""
    buf = np.frombuffer(memoryview(data).cast('B'), dtype=np.uint8)
    reg = crc ^ 0xffffffff
    n = buf.size // _CHUNK
    if n >= 4:
        cols = np.ascontiguousarray(buf[:n * _CHUNK].reshape(n, _CHUNK).T)
        s = np.zeros(n, dtype=np.uint32)
        for j in range(_CHUNK):
            s = _TABLE[(s ^ cols[j]) & 0xff] ^ (s >> 8)
        t0, t1, t2, t3 = _SHIFT_CHUNK
        for c in s.tolist():
            reg = t0[reg & 0xff] ^ t1[(reg >> 8) & 0xff] ^ t2[(reg >> 16) & 0xff] ^ t3[reg >> 24] ^ c
        tail = buf[n * _CHUNK:]
    else:
        tail = buf
    return _crc_bytes(reg, tail.tobytes()) ^ 0xffffffff


def mask_crc(c):
    return ((((c >> 15) | (c << 17)) & 0xffffffff) + MASK_DELTA) & 0xffffffff


def unmask_crc(m):
    r = (m - MASK_DELTA) & 0xffffffff
    return ((r >> 17) | (r << 15)) & 0xffffffff


# ---------------------------------------------------------------------------------------------------------- varints / protobuf
def put_varint(v):
    v &= 0xffffffffffffffff                                         # negative int64 -> ten-byte two's complement
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7f) | 0x80); v >>= 7
    out.append(v)
    return bytes(out)


def get_varint(buf, pos, path='<buffer>', what='varint'):
    v, shift = 0, 0
    while True:
        if pos >= len(buf):
            raise CheckpointFormatError(path, 'truncated %s' % what)
        b = buf[pos]; pos += 1
        v |= (b & 0x7f) << shift
        if not b & 0x80:
            return v, pos
        shift += 7
        if shift > 63:
            raise CheckpointFormatError(path, 'overlong %s' % what)


def _fixed32(buf, pos):
    return int.from_bytes(buf[pos:pos + 4], 'little')


def parse_fields(buf, path, what):
    """Protobuf wire format -> list of (field number, wire type, value): varints as unsigned ints, fixed32 / fixed64 as
    unsigned ints, length-delimited as bytes.  Groups (wire types 3, 4) are refused."""
    out, pos, n = [], 0, len(buf)
    while pos < n:
        key, pos = get_varint(buf, pos, path, what)
        field, wt = key >> 3, key & 7
        if wt == 0:
            v, pos = get_varint(buf, pos, path, what)
        elif wt == 1:
            if pos + 8 > n:
                raise CheckpointFormatError(path, 'truncated %s' % what)
            v = int.from_bytes(buf[pos:pos + 8], 'little'); pos += 8
        elif wt == 2:
            ln, pos = get_varint(buf, pos, path, what)
            if pos + ln > n:
                raise CheckpointFormatError(path, 'truncated %s' % what)
            v = bytes(buf[pos:pos + ln]); pos += ln
        elif wt == 5:
            if pos + 4 > n:
                raise CheckpointFormatError(path, 'truncated %s' % what)
            v = _fixed32(buf, pos); pos += 4
        else:
            raise CheckpointFormatError(path, 'unsupported wire type %d in %s' % (wt, what))
        out.append((field, wt, v))
    return out


def _int64(v):
    return v - (1 << 64) if v >= 1 << 63 else v


def _pb_varint(field, v):
    return put_varint(field << 3) + put_varint(v)


def _pb_bytes(field, b):
    return put_varint((field << 3) | 2) + put_varint(len(b)) + b


def _pb_fixed32(field, v):
    return put_varint((field << 3) | 5) + int(v).to_bytes(4, 'little')


def encode_header(num_shards=1, endianness=0, producer=1):
    out = b''
    if num_shards:
        out += _pb_varint(1, num_shards)
    if endianness:
        out += _pb_varint(2, endianness)
    return out + _pb_bytes(3, _pb_varint(1, producer))


def encode_entry(dtype_id, shape, shard_id, offset, size, crc_masked):
    shp = b''.join(_pb_bytes(2, _pb_varint(1, int(d))) for d in shape)
    out = _pb_varint(1, dtype_id) + _pb_bytes(2, shp)
    if shard_id:
        out += _pb_varint(3, shard_id)
    if offset:
        out += _pb_varint(4, offset)
    if size:
        out += _pb_varint(5, size)
    return out + _pb_fixed32(6, crc_masked)


def decode_header(buf, path):
    h = {'num_shards': 0, 'endianness': 0, 'producer': 0}
    for f, wt, v in parse_fields(buf, path, 'BundleHeaderProto'):
        if f == 1 and wt == 0:
            h['num_shards'] = _int64(v)
        elif f == 2 and wt == 0:
            h['endianness'] = v
        elif f == 3 and wt == 2:
            for f2, wt2, v2 in parse_fields(v, path, 'VersionDef'):
                if f2 == 1 and wt2 == 0:
                    h['producer'] = _int64(v2)
    return h


def decode_entry(buf, path, name):
    e = {'dtype': 0, 'shape': [], 'shard_id': 0, 'offset': 0, 'size': 0, 'crc32c': None, 'n_slices': 0}
    what = 'BundleEntryProto of %r' % name
    for f, wt, v in parse_fields(buf, path, what):
        if f == 1 and wt == 0:
            e['dtype'] = v
        elif f == 2 and wt == 2:
            for f2, wt2, v2 in parse_fields(v, path, what):
                if f2 == 2 and wt2 == 2:
                    size = 0
                    for f3, wt3, v3 in parse_fields(v2, path, what):
                        if f3 == 1 and wt3 == 0:
                            size = _int64(v3)
                    e['shape'].append(size)
                elif f2 == 3 and wt2 == 0 and v2:
                    raise CheckpointFormatError(path, '%r has an unknown-rank shape' % name)
        elif f == 3 and wt == 0:
            e['shard_id'] = _int64(v)
        elif f == 4 and wt == 0:
            e['offset'] = _int64(v)
        elif f == 5 and wt == 0:
            e['size'] = _int64(v)
        elif f == 6 and wt == 5:
            e['crc32c'] = v
        elif f == 7 and wt == 2:
            e['n_slices'] += 1
    return e


# ---------------------------------------------------------------------------------------------------------- LevelDB table
def _read_block(data, offset, size, path, what):
    end = offset + size
    if offset < 0 or size < 0 or end + BLOCK_TRAILER > len(data):
        raise CheckpointFormatError(path, 'truncated: %s block [%d, +%d) runs past the end of the file' % (what, offset, size))
    contents = data[offset:end]
    btype = data[end]
    stored = _fixed32(data, end + 1)
    if crc32c(data[offset:end + 1]) != unmask_crc(stored):
        raise CheckpointFormatError(path, 'block crc mismatch in the %s block at offset %d' % (what, offset))
    if btype == 1:
        raise CheckpointFormatError(path, 'snappy-compressed %s block at offset %d is not supported' % (what, offset))
    if btype != 0:
        raise CheckpointFormatError(path, 'unknown block type %d of the %s block at offset %d' % (btype, what, offset))
    return contents


def _block_entries(block, path, what):
    """-> list of (key bytes, value bytes) of one block."""
    if len(block) < 4:
        raise CheckpointFormatError(path, 'truncated %s block' % what)
    n_restarts = _fixed32(block, len(block) - 4)
    limit = len(block) - 4 - 4 * n_restarts
    if n_restarts < 1 or limit < 0:
        raise CheckpointFormatError(path, 'bad restart array in a %s block' % what)
    out, pos, key = [], 0, b''
    while pos < limit:
        shared, pos = get_varint(block, pos, path, what + ' entry')
        non_shared, pos = get_varint(block, pos, path, what + ' entry')
        vlen, pos = get_varint(block, pos, path, what + ' entry')
        if shared > len(key) or pos + non_shared + vlen > limit:
            raise CheckpointFormatError(path, 'corrupt entry in a %s block' % what)
        key = key[:shared] + bytes(block[pos:pos + non_shared]); pos += non_shared
        out.append((key, bytes(block[pos:pos + vlen]))); pos += vlen
    return out


def _decode_handle(buf, pos, path):
    off, pos = get_varint(buf, pos, path, 'BlockHandle')
    size, pos = get_varint(buf, pos, path, 'BlockHandle')
    return off, size, pos


def read_table(path):
    """All (key, value) pairs of a LevelDB-format table file, in file order."""
    with open(path, 'rb') as f:
        data = f.read()
    if len(data) < FOOTER_LEN:
        raise CheckpointFormatError(path, 'truncated: %d bytes, shorter than the %d-byte footer' % (len(data), FOOTER_LEN))
    footer = data[-FOOTER_LEN:]
    if int.from_bytes(footer[40:48], 'little') != TABLE_MAGIC:
        raise CheckpointFormatError(path, 'bad magic 0x%016x (not a table: V1 checkpoint or other file?)' % int.from_bytes(footer[40:48], 'little'))
    _, _, p = _decode_handle(footer, 0, path)                       # metaindex: no filter or stats blocks are used
    ioff, isize, _ = _decode_handle(footer, p, path)
    body = data[:-FOOTER_LEN]
    out = []
    for sep, handle in _block_entries(_read_block(body, ioff, isize, path, 'index'), path, 'index'):
        doff, dsize, _ = _decode_handle(handle, 0, path)
        out += _block_entries(_read_block(body, doff, dsize, path, 'data'), path, 'data')
    return out


def _build_block(entries, restart_interval):
    buf, restarts, prev = bytearray(), [], b''
    for i, (k, v) in enumerate(entries):
        if i % restart_interval == 0:
            restarts.append(len(buf)); shared = 0
        else:
            shared = 0
            while shared < min(len(prev), len(k)) and prev[shared] == k[shared]:
                shared += 1
        buf += put_varint(shared) + put_varint(len(k) - shared) + put_varint(len(v)) + k[shared:] + v
        prev = k
    if not restarts:
        restarts = [0]
    for r in restarts:
        buf += r.to_bytes(4, 'little')
    buf += len(restarts).to_bytes(4, 'little')
    return bytes(buf)


def _emit_block(out, contents):
    handle = put_varint(len(out)) + put_varint(len(contents))
    out += contents + b'\x00' + mask_crc(crc32c(contents + b'\x00')).to_bytes(4, 'little')
    return handle


def build_table(entries, block_size=262144):
    """entries: (key bytes, value bytes) in strictly increasing bytewise key order -> bytes of the table file."""
    keys = [k for k, _ in entries]
    if any(a >= b for a, b in zip(keys, keys[1:])):
        raise ValueError('table keys must be unique and in bytewise order')
    out, index, cur, cur_size = bytearray(), [], [], 0
    for i, (k, v) in enumerate(entries):
        cur.append((k, v)); cur_size += len(k) + len(v) + 8
        if cur_size >= block_size or i == len(entries) - 1:
            index.append((cur[-1][0], _emit_block(out, _build_block(cur, 16))))     # separator: the block's last key
            cur, cur_size = [], 0
    meta = _emit_block(out, _build_block([], 16))
    idx = _emit_block(out, _build_block(index, 1))
    footer = (meta + idx).ljust(40, b'\x00') + TABLE_MAGIC.to_bytes(8, 'little')
    return bytes(out + footer)


# ---------------------------------------------------------------------------------------------------------- bundles
def data_path(prefix, shard=0, num_shards=1):
    return '%s.data-%05d-of-%05d' % (prefix, shard, num_shards)


def _read_index(prefix):
    path = prefix + '.index'
    if not os.path.exists(path):
        raise CheckpointFormatError(path, 'missing index file (a V2 checkpoint prefix is expected, not a V1 file or .meta graph)')
    rows = read_table(path)
    if not rows or rows[0][0] != b'':
        raise CheckpointFormatError(path, 'no BundleHeaderProto under the empty key')
    keys = [k for k, _ in rows]
    if any(a >= b for a, b in zip(keys, keys[1:])):
        raise CheckpointFormatError(path, 'keys are not in bytewise order')
    h = decode_header(rows[0][1], path)
    if h['num_shards'] != 1:
        raise CheckpointFormatError(path, 'sharded bundle (num_shards = %d): only single-shard checkpoints are supported' % h['num_shards'])
    if h['endianness'] != 0:
        raise CheckpointFormatError(path, 'big-endian bundle is not supported')
    entries = OrderedDict()
    for k, v in rows[1:]:
        name = k.decode('utf-8')
        e = decode_entry(v, path, name)
        if e['n_slices']:
            raise CheckpointFormatError(path, 'sliced (partitioned) variable %r is not supported' % name)
        if e['dtype'] not in DTYPES:
            raise CheckpointFormatError(path, 'unsupported dtype %d of %r (DT_FLOAT, DT_DOUBLE, DT_INT32, DT_INT64 only)' % (e['dtype'], name))
        if e['shard_id'] != 0:
            raise CheckpointFormatError(path, '%r lives in shard %d of a single-shard bundle' % (name, e['shard_id']))
        if any(d < 0 for d in e['shape']):
            raise CheckpointFormatError(path, '%r has a partially known shape %s' % (name, e['shape']))
        n = int(np.prod(e['shape'], dtype=np.int64)) * DTYPES[e['dtype']].itemsize
        if n != e['size']:
            raise CheckpointFormatError(path, '%r: size %d does not match dtype and shape %s' % (name, e['size'], e['shape']))
        entries[name] = e
    return path, entries


def list_checkpoint(prefix):
    """-> {variable name: (numpy dtype, shape tuple)} from the index alone."""
    _, entries = _read_index(prefix)
    return OrderedDict((n, (DTYPES[e['dtype']], tuple(e['shape']))) for n, e in entries.items())


def read_checkpoint(prefix):
    """-> OrderedDict variable name -> ndarray (little-endian dtypes, C order), every tensor's crc32c verified."""
    _, entries = _read_index(prefix)
    dpath = data_path(prefix)
    if not os.path.exists(dpath):
        raise CheckpointFormatError(dpath, 'missing data file')
    with open(dpath, 'rb') as f:
        data = f.read()
    out = OrderedDict()
    for name, e in entries.items():
        o, n = e['offset'], e['size']
        if o < 0 or o + n > len(data):
            raise CheckpointFormatError(dpath, 'truncated: %r needs bytes [%d, %d) of %d' % (name, o, o + n, len(data)))
        raw = data[o:o + n]
        if e['crc32c'] is not None and crc32c(raw) != unmask_crc(e['crc32c']):
            raise CheckpointFormatError(dpath, 'tensor crc mismatch for %r' % name)
        out[name] = np.frombuffer(raw, dtype=DTYPES[e['dtype']]).reshape(e['shape']).copy()
    return out


def write_checkpoint(prefix, tensors, block_size=262144, write_state=True):
    """tensors: {name: array-like} (float32, float64, int32 or int64) -> <prefix>.index + <prefix>.data-00000-of-00001, and
    the directory's `checkpoint` state file pointing at <prefix> (as Saver.save leaves it).  Returns the prefix."""
    arrs = {}
    for name, a in tensors.items():
        a = np.asarray(a)
        if a.dtype not in DTYPE_IDS:
            raise TypeError('%s: dtype %s has no DT_ mapping here (float32, float64, int32, int64)' % (name, a.dtype))
        if not name or name.endswith(':0'):
            raise ValueError('variable names are stored without the :0 output suffix, got %r' % name)
        arrs[name] = np.array(a, dtype=a.dtype.newbyteorder('<'), order='C')            # ascontiguousarray would make a scalar 1-d
    d = os.path.dirname(prefix)
    if d:
        os.makedirs(d, exist_ok=True)
    rows, off = [(b'', encode_header())], 0
    with open(data_path(prefix), 'wb') as f:
        for name in sorted(arrs, key=lambda s: s.encode('utf-8')):
            a = arrs[name]
            raw = a.tobytes()
            f.write(raw)
            rows.append((name.encode('utf-8'), encode_entry(DTYPE_IDS[a.dtype.newbyteorder('=')], a.shape, 0, off, len(raw), mask_crc(crc32c(raw)))))
            off += len(raw)
    with open(prefix + '.index', 'wb') as f:
        f.write(build_table(rows, block_size))
    if write_state:
        write_checkpoint_state(d or '.', prefix)
    return prefix


def write_checkpoint_state(directory, prefix):
    """The text CheckpointState Saver.save keeps in <directory>/checkpoint (relative path when <prefix> lives there)."""
    rel = os.path.relpath(prefix, directory) if os.path.dirname(os.path.abspath(prefix)) == os.path.abspath(directory) else prefix
    esc = rel.replace('\\', '\\\\').replace('"', '\\"')
    with open(os.path.join(directory, STATE_FILE), 'w') as f:
        f.write('model_checkpoint_path: "%s"\nall_model_checkpoint_paths: "%s"\n' % (esc, esc))


def latest_checkpoint(directory):
    """tf.train.latest_checkpoint: the prefix named by model_checkpoint_path in <directory>/checkpoint, or None when the state
    file or the bundle it names is absent.  A relative path is taken from <directory>; an absolute path that no longer exists
    (a run moved from another machine) falls back to its base name inside <directory>."""
    sf = os.path.join(directory, STATE_FILE)
    if not os.path.exists(sf):
        return None
    m = re.search(r'^\s*model_checkpoint_path\s*:\s*"((?:[^"\\]|\\.)*)"', open(sf).read(), re.M)
    if not m:
        return None
    p = re.sub(r'\\(.)', r'\1', m.group(1))
    cands = [p] if os.path.isabs(p) else [os.path.join(directory, p)]
    cands.append(os.path.join(directory, os.path.basename(p)))
    for c in cands:
        if os.path.exists(c + '.index'):
            return c
    return None
