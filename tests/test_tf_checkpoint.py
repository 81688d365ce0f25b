"""TF tensor-bundle V2 reader / writer (me-trpo_amd/tf_checkpoint.py), rllab policy pickles, and the status codes of the
optimizer-state entry points: host logic, runs without a GPU."""
import ctypes as C
import os
import pickle
import struct
import sys
import types

import numpy as np
import pytest


def _tfc():
    from metrpo_amd import tf_checkpoint
    return tf_checkpoint


# ---------------------------------------------------------------------------------------------------------- crc32c
def test_crc32c_rfc3720_vectors():
    T = _tfc()
    assert T.crc32c(b'\x00' * 32) == 0x8a9136aa
    assert T.crc32c(b'\xff' * 32) == 0x62a8ab43
    assert T.crc32c(bytes(range(32))) == 0x46dd794e
    assert T.crc32c(bytes(range(31, -1, -1))) == 0x113fdb5c
    assert T.crc32c(b'123456789') == 0xe3069283
    assert T.crc32c_bytewise(b'123456789') == 0xe3069283


def test_crc_mask_and_unmask():
    T = _tfc()
    c = 0xe3069283
    rot = ((c >> 15) | (c << 17)) & 0xffffffff
    assert T.mask_crc(c) == (rot + 0xa282ead8) & 0xffffffff
    rng = np.random.RandomState(0)
    for c in [0, 1, 0xffffffff, 0x80000000] + [int(x) for x in rng.randint(0, 2 ** 32, 200, dtype=np.uint64)]:
        assert T.unmask_crc(T.mask_crc(c)) == c
        assert T.mask_crc(T.unmask_crc(c)) == c


def test_vectorised_crc_equals_bytewise():
    T = _tfc()
    rng = np.random.RandomState(1)
    lengths = [0, 1, 4095, 4096, 4 * 4096 - 1, 4 * 4096, 4 * 4096 + 1, 100000] + [int(n) for n in rng.randint(0, 100001, 12)]
    for n in lengths:
        d = rng.randint(0, 256, n).astype(np.uint8).tobytes()
        assert T.crc32c(d) == T.crc32c_bytewise(d), n
    d = rng.randint(0, 256, 50000).astype(np.uint8).tobytes()
    assert T.crc32c(d[20000:], T.crc32c(d[:20000])) == T.crc32c(d)            # continuation


# ---------------------------------------------------------------------------------------------------------- hand-assembled index
def _varint(v):
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7f) | 0x80); v >>= 7
    out.append(v)
    return bytes(out)


def _masked_crc(b):
    T = _tfc()
    c = T.crc32c_bytewise(b)
    return ((((c >> 15) | (c << 17)) & 0xffffffff) + 0xa282ead8) & 0xffffffff


def _block(entries):
    """one restart point at 0, all later keys prefix-compressed against their predecessor (written out by hand)."""
    body, prev = b'', b''
    for k, v in entries:
        shared = 0
        while shared < min(len(prev), len(k)) and prev[shared] == k[shared]:
            shared += 1
        if not body:
            shared = 0
        body += _varint(shared) + _varint(len(k) - shared) + _varint(len(v)) + k[shared:] + v
        prev = k
    return body + struct.pack('<I', 0) + struct.pack('<I', 1)


def _hand_bundle(tmp_path, extra_entry_fields=b'', num_shards=1, endianness=0):
    """A one-data-block index and its data file, every byte laid down from the format spec."""
    a = np.arange(6, dtype='<f4').reshape(2, 3)
    b = np.array([7, -8], dtype='<i8')
    data = a.tobytes() + b.tobytes()
    hdr = b'\x08' + _varint(num_shards) + (b'\x10' + _varint(endianness) if endianness else b'') + b'\x1a\x02\x08\x01'

    def entry(dtype, dims, off, size, raw):
        shp = b''.join(b'\x12' + _varint(len(b'\x08' + _varint(d))) + b'\x08' + _varint(d) for d in dims)
        e = b'\x08' + _varint(dtype) + b'\x12' + _varint(len(shp)) + shp
        if off:
            e += b'\x20' + _varint(off)
        e += b'\x28' + _varint(size) + b'\x35' + struct.pack('<I', _masked_crc(raw))
        return e + extra_entry_fields
    rows = [(b'', hdr), (b'model/a', entry(1, [2, 3], 0, 24, a.tobytes())), (b'model/b', entry(9, [2], 24, 16, b.tobytes()))]
    f = b''
    dblock = _block(rows)
    d_off, d_size = len(f), len(dblock)
    f += dblock + b'\x00' + struct.pack('<I', _masked_crc(dblock + b'\x00'))
    mblock = struct.pack('<I', 0) + struct.pack('<I', 1)
    m_off, m_size = len(f), len(mblock)
    f += mblock + b'\x00' + struct.pack('<I', _masked_crc(mblock + b'\x00'))
    iblock = _block([(b'model/b', _varint(d_off) + _varint(d_size))])
    i_off, i_size = len(f), len(iblock)
    f += iblock + b'\x00' + struct.pack('<I', _masked_crc(iblock + b'\x00'))
    handles = _varint(m_off) + _varint(m_size) + _varint(i_off) + _varint(i_size)
    f += handles + b'\x00' * (40 - len(handles)) + struct.pack('<Q', 0xdb4775248b80fb57)
    prefix = str(tmp_path / 'hand.ckpt')
    open(prefix + '.index', 'wb').write(f)
    open(prefix + '.data-00000-of-00001', 'wb').write(data)
    return prefix, {'model/a': a, 'model/b': b}


def test_reader_parses_a_hand_assembled_index(tmp_path):
    T = _tfc()
    prefix, want = _hand_bundle(tmp_path)
    got = T.read_checkpoint(prefix)
    assert list(got) == ['model/a', 'model/b']
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape
        assert got[k].tobytes() == want[k].tobytes()
    assert T.list_checkpoint(prefix) == {'model/a': (np.dtype('<f4'), (2, 3)), 'model/b': (np.dtype('<i8'), (2,))}


# ---------------------------------------------------------------------------------------------------------- writer round trip
def _tensors():
    rng = np.random.RandomState(2)
    t = {}
    for dt in (np.float32, np.float64, np.int32, np.int64):
        n = np.dtype(dt).name
        t['scope/%s/scalar' % n] = np.array(rng.randn() * 100).astype(dt)
        t['scope/%s/empty' % n] = np.zeros((0,), dt)
        t['scope/%s/mat' % n] = (rng.randn(3, 5) * 1000).astype(dt)
    t['scope/float32/special'] = np.array([np.nan, np.inf, -np.inf, -0.0, 1e-45], np.float32)
    for i in range(40):                                                  # long shared prefixes across many blocks
        t['training_dynamics/model%d/layer0/weights' % i] = rng.randn(2, 3).astype(np.float32)
    return t


def test_round_trip_many_blocks_all_dtypes(tmp_path):
    T = _tfc()
    t = _tensors()
    prefix = str(tmp_path / 'sub' / 'rt.ckpt')
    T.write_checkpoint(prefix, t, block_size=64)
    rows = T.read_table(prefix + '.index')
    got = T.read_checkpoint(prefix)
    assert set(got) == set(t)
    for k, a in t.items():
        assert got[k].dtype == a.dtype and got[k].shape == a.shape, k
        assert got[k].tobytes() == a.tobytes(), k
    # many data blocks -> a multi-entry index, every block's first entry a restart point (shared = 0)
    data = open(prefix + '.index', 'rb').read()
    footer = data[-48:]
    _, _, p = T._decode_handle(footer, 0, 'f')
    ioff, isize, _ = T._decode_handle(footer, p, 'f')
    index = T._block_entries(T._read_block(data[:-48], ioff, isize, 'f', 'index'), 'f', 'index')
    assert len(index) > 10 and len(rows) == len(t) + 1
    assert all(T.get_varint(data, T._decode_handle(h, 0, 'f')[0])[0] == 0 for _, h in index)
    # one big block: entries between restart points (every 16th) share a prefix with their predecessor
    T.write_checkpoint(str(tmp_path / 'one.ckpt'), t, write_state=False)
    data = open(str(tmp_path / 'one.ckpt.index'), 'rb').read()
    size = _first_block_size(T, data)
    assert len(T._block_entries(T._read_block(data[:-48], 0, size, 'f', 'data'), 'f', 'data')) == len(t) + 1
    shared, q = [], 0
    limit = size - 4 - 4 * struct.unpack('<I', data[size - 4:size])[0]
    while q < limit:
        sh, q = T.get_varint(data, q); nsh, q = T.get_varint(data, q); vl, q = T.get_varint(data, q)
        shared.append(sh); q += nsh + vl
    assert struct.unpack('<I', data[size - 4:size])[0] == (len(t) + 1 + 15) // 16
    assert shared[0] == shared[16] == shared[32] == 0
    assert sum(sh > 0 for sh in shared) > len(t) // 2
    assert T.latest_checkpoint(str(tmp_path / 'sub')) == prefix


def _first_block_size(T, data):
    footer = data[-48:]
    _, _, p = T._decode_handle(footer, 0, 'f')
    ioff, isize, _ = T._decode_handle(footer, p, 'f')
    index = T._block_entries(T._read_block(data[:-48], ioff, isize, 'f', 'index'), 'f', 'index')
    return T._decode_handle(index[0][1], 0, 'f')[1]


def test_key_order_header_first_then_bytewise(tmp_path):
    T = _tfc()
    t = {'b': np.ones(1, np.float32), 'a/z': np.ones(1, np.float32), 'a/B': np.ones(1, np.float32), 'a_': np.ones(1, np.float32),
         'A': np.ones(1, np.float32)}
    prefix = str(tmp_path / 'order.ckpt')
    T.write_checkpoint(prefix, t, block_size=32)
    keys = [k for k, _ in T.read_table(prefix + '.index')]
    assert keys[0] == b''
    assert keys[1:] == sorted(k.encode() for k in t)
    assert keys[1:] == [b'A', b'a/B', b'a/z', b'a_', b'b']
    with pytest.raises(ValueError):
        T.build_table([(b'b', b''), (b'a', b'')])


def test_checkpoint_state_file(tmp_path):
    T = _tfc()
    assert T.latest_checkpoint(str(tmp_path)) is None
    p = T.write_checkpoint(str(tmp_path / 'policy-and-models-3.ckpt'), {'x': np.zeros(2, np.float32)})
    txt = open(str(tmp_path / 'checkpoint')).read()
    assert 'model_checkpoint_path: "policy-and-models-3.ckpt"' in txt
    assert T.latest_checkpoint(str(tmp_path)) == p
    # a run moved from another machine: the absolute path it recorded no longer exists, the base name next to the state file does
    open(str(tmp_path / 'checkpoint'), 'w').write('model_checkpoint_path: "/gone/run/policy-and-models-3.ckpt"\n'
                                                 'all_model_checkpoint_paths: "/gone/run/policy-and-models-3.ckpt"\n')
    assert T.latest_checkpoint(str(tmp_path)) == p


# ---------------------------------------------------------------------------------------------------------- refusals
def _good(tmp_path, name='g.ckpt'):
    T = _tfc()
    prefix = str(tmp_path / name)
    T.write_checkpoint(prefix, {'v/a': np.arange(40, dtype=np.float32), 'v/b': np.arange(3, dtype=np.int32)}, write_state=False)
    return prefix


def _raises(prefix, match):
    T = _tfc()
    with pytest.raises(T.CheckpointFormatError, match=match) as e:
        T.read_checkpoint(prefix)
    assert os.path.basename(e.value.path).startswith(os.path.basename(prefix))
    return e.value


def test_truncated_index_and_data(tmp_path):
    p = _good(tmp_path)
    idx = open(p + '.index', 'rb').read()
    open(p + '.index', 'wb').write(idx[:30])
    _raises(p, 'truncated')
    p = _good(tmp_path, 'g2.ckpt')
    idx = open(p + '.index', 'rb').read()
    open(p + '.index', 'wb').write(idx[20:])               # footer intact, blocks shifted: a handle runs past the end or its crc fails
    with pytest.raises(_tfc().CheckpointFormatError):
        _tfc().read_checkpoint(p)
    p = _good(tmp_path, 'g3.ckpt')
    d = open(p + '.data-00000-of-00001', 'rb').read()
    open(p + '.data-00000-of-00001', 'wb').write(d[:100])
    _raises(p, 'truncated')


def test_flipped_bytes(tmp_path):
    p = _good(tmp_path)
    idx = bytearray(open(p + '.index', 'rb').read())
    idx[3] ^= 0x40                                          # inside the first data block
    open(p + '.index', 'wb').write(bytes(idx))
    _raises(p, 'block crc mismatch')
    p = _good(tmp_path, 'g2.ckpt')
    d = bytearray(open(p + '.data-00000-of-00001', 'rb').read())
    d[5] ^= 0x01
    open(p + '.data-00000-of-00001', 'wb').write(bytes(d))
    e = _raises(p, 'tensor crc mismatch')
    assert "'v/a'" in str(e)


def test_wrong_magic_and_missing_files(tmp_path):
    p = _good(tmp_path)
    idx = bytearray(open(p + '.index', 'rb').read())
    idx[-1] ^= 0xff
    open(p + '.index', 'wb').write(bytes(idx))
    _raises(p, 'bad magic')
    p = _good(tmp_path, 'g2.ckpt')
    os.remove(p + '.data-00000-of-00001')
    _raises(p, 'missing data file')
    _raises(str(tmp_path / 'nothing.ckpt'), 'missing index file')


def test_two_shards_sliced_big_endian_snappy_and_dtype(tmp_path):
    T = _tfc()
    prefix, _ = _hand_bundle(tmp_path, num_shards=2)
    _raises(prefix, 'sharded bundle')
    prefix, _ = _hand_bundle(tmp_path, extra_entry_fields=b'\x3a\x00')           # field 7 (slices), an empty TensorSliceProto
    _raises(prefix, r'sliced \(partitioned\) variable')
    prefix, _ = _hand_bundle(tmp_path, endianness=1)
    _raises(prefix, 'big-endian')
    rows = [(b'', T.encode_header()), (b'x', T.encode_entry(7, [1], 0, 0, 1, 0))]      # DT_STRING
    open(str(tmp_path / 's.ckpt.index'), 'wb').write(T.build_table(rows))
    open(str(tmp_path / 's.ckpt.data-00000-of-00001'), 'wb').write(b'')
    _raises(str(tmp_path / 's.ckpt'), 'unsupported dtype 7')
    # a snappy block: type byte 1 with a correct crc
    blk = T._build_block([(b'', T.encode_header())], 16)
    f = bytearray(blk + b'\x01' + struct.pack('<I', T.mask_crc(T.crc32c(blk + b'\x01'))))
    meta = T._emit_block(f, T._build_block([], 16))
    idx = T._emit_block(f, T._build_block([(b'', T.put_varint(0) + T.put_varint(len(blk)))], 1))
    f += (meta + idx).ljust(40, b'\x00') + struct.pack('<Q', T.TABLE_MAGIC)
    open(str(tmp_path / 'z.ckpt.index'), 'wb').write(bytes(f))
    _raises(str(tmp_path / 'z.ckpt'), 'snappy')
    with pytest.raises(TypeError):
        T.write_checkpoint(str(tmp_path / 'c.ckpt'), {'c': np.zeros(2, np.complex64)})


# ---------------------------------------------------------------------------------------------------------- Adam step from beta powers
def test_adam_step_from_beta_powers():
    from metrpo_amd import formats as F
    # pinned by literals: TF's adam.py creates beta1_power = beta1 and multiplies it by beta1 after each step, so a fresh
    # optimizer (no step yet) holds (beta1, beta2) and one that took t steps holds (beta1^(t+1), beta2^(t+1))
    assert F.adam_step_from_powers(np.float32(0.9), np.float32(0.999)) == 0
    assert F.adam_step_from_powers(np.float32(0.81), np.float32(0.998001)) == 1
    assert F.adam_step_from_powers(np.float32(0.9 ** 4), np.float32(0.999 ** 4)) == 3
    assert F.adam_step_from_powers(np.float32(0.6561), np.float32(0.996006)) == 3
    assert F._beta_powers(0, 0.9, 0.999) == (np.float32(0.9), np.float32(0.999))
    assert F._beta_powers(3, 0.9, 0.999) == (np.float32(0.6561), np.float32(0.999 ** 4))
    for t in (0, 1, 3, 50, 700):
        b1, b2 = F._beta_powers(t, 0.9, 0.999)
        assert F.adam_step_from_powers(b1, b2) == t
    b1, b2 = F._beta_powers(5000, 0.9, 0.999)                # beta1_power has underflowed float32
    assert b1 == 0.0 and F.adam_step_from_powers(b1, b2) == 5000
    with pytest.raises(F.OptimizerStateError):
        F.adam_step_from_powers(np.float32(0.9 ** 4), np.float32(0.999 ** 9))


# ---------------------------------------------------------------------------------------------------------- C entry points
def test_optimizer_state_entry_points_reject_null_without_gpu():
    from metrpo_amd import _lib
    lib = _lib.lib
    t = C.c_int64(7)
    assert lib.metrpo_get_dyn_adam(None, None, None, C.byref(t), None) == -1            # METRPO_EINVAL
    assert lib.metrpo_set_dyn_adam(None, None, None, 0, None) == -1
    assert lib.metrpo_get_policy_adam(None, None, None, C.byref(t), None) == -1
    assert lib.metrpo_set_policy_adam(None, None, None, 0, None) == -1
    assert t.value == 7


# ---------------------------------------------------------------------------------------------------------- rllab pickles
class _Stub(object):
    """What rllab's Serializable + Parameterized leave in a pickle: __args, __kwargs and the flat params vector."""

    def __init__(self, params, kwargs):
        self._state = {'__args': (), '__kwargs': kwargs, 'params': params}

    def __getstate__(self):
        return self._state

    def __setstate__(self, d):
        self._state = d


def _fake_rllab_modules():
    names = ['sandbox', 'sandbox.rocky', 'sandbox.rocky.tf', 'sandbox.rocky.tf.policies', 'sandbox.rocky.tf.policies.gaussian_mlp_policy',
             'tensorflow', 'tensorflow.python', 'tensorflow.python.ops', 'tensorflow.python.ops.array_ops']
    mods = {n: types.ModuleType(n) for n in names}
    cls = type('GaussianMLPPolicy', (_Stub,), {'__module__': 'sandbox.rocky.tf.policies.gaussian_mlp_policy'})
    mods['sandbox.rocky.tf.policies.gaussian_mlp_policy'].GaussianMLPPolicy = cls

    def identity(x):
        return x
    identity.__module__, identity.__qualname__ = 'tensorflow.python.ops.array_ops', 'identity'
    mods['tensorflow.python.ops.array_ops'].identity = identity
    return mods, cls, identity


def _dump_policy(path, use_joblib):
    theta = np.random.RandomState(3).randn(10 * 32 + 32 + 32 * 32 + 32 + 32 * 2 + 2 + 2)
    mods, cls, identity = _fake_rllab_modules()
    saved = {n: sys.modules.get(n) for n in mods}
    sys.modules.update(mods)
    try:
        obj = cls(theta, {'name': 'training_policy', 'hidden_sizes': (32, 32), 'init_std': 1.0, 'output_nonlinearity': identity})
        if use_joblib:
            import joblib
            joblib.dump(obj, path)
        else:
            with open(path, 'wb') as f:
                pickle.dump(obj, f, protocol=2)
    finally:
        for n, m in saved.items():
            if m is None:
                sys.modules.pop(n, None)
            else:
                sys.modules[n] = m
    return theta


@pytest.mark.parametrize('use_joblib', [True, False])
def test_rllab_policy_pickle_loads_without_rllab(tmp_path, use_joblib):
    if use_joblib:
        pytest.importorskip('joblib')
    from metrpo_amd import formats
    path = str(tmp_path / 'params.pkl')
    theta = _dump_policy(path, use_joblib)
    assert 'sandbox.rocky.tf.policies.gaussian_mlp_policy' not in sys.modules
    got, meta = formats.load_rllab_policy_pickle(path)
    assert got.dtype == np.float32 and got.shape == theta.shape
    np.testing.assert_array_equal(got, theta.astype(np.float32))
    assert meta['hidden_sizes'] == (32, 32) and meta['init_std'] == 1.0
    assert meta['class'] == 'sandbox.rocky.tf.policies.gaussian_mlp_policy.GaussianMLPPolicy'


class _Payload(object):
    """An object whose unpickling would call a builtin outside the allow-list."""

    def __reduce__(self):
        return (print, ('payload ran',))


def test_joblib_object_array_payload_goes_through_the_restricted_unpickler(tmp_path, capsys):
    """joblib writes an object-dtype array as a nested pickle that its own reader loads with a plain pickle.load: the
    container must not open a way around find_class."""
    joblib = pytest.importorskip('joblib')
    from metrpo_amd import formats
    evil = np.empty(2, dtype=object)
    evil[0], evil[1] = 'x', _Payload()
    path = str(tmp_path / 'params.pkl')
    joblib.dump({'params': np.zeros(3), 'x': evil}, path)
    with pytest.raises(pickle.UnpicklingError, match='builtins.print'):
        formats.load_rllab_policy_pickle(path)
    assert 'payload ran' not in capsys.readouterr().out
    ok = np.empty(2, dtype=object)
    ok[0], ok[1] = 'tanh', (32, 32)
    joblib.dump({'params': np.arange(4.0), 'x': ok}, path)             # harmless object arrays still load
    theta, _ = formats.load_rllab_policy_pickle(path)
    np.testing.assert_array_equal(theta, np.arange(4, dtype=np.float32))


def test_pickle_naming_os_system_is_refused(tmp_path):
    from metrpo_amd import formats
    path = str(tmp_path / 'evil.pkl')
    with open(path, 'wb') as f:
        f.write(b'cos\nsystem\n(S"echo pwned"\ntR.')
    with pytest.raises(pickle.UnpicklingError, match='os.system'):
        formats.load_rllab_policy_pickle(path)
