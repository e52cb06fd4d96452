"""A small read-only HDF5 reader for basecaller trace files (Flappie `--trace` .hdf5, Guppy flip-flop .fast5).

The reference reads these with h5py (decode.py:53-65,89-104): `hdf[first_read_id]['trace']` for Flappie,
`/Analyses/Basecall_1D_000/BaseCalled_template/Trace` for Guppy — uint8 (T, 8) flip-flop state posteriors.  h5py is
not a dependency of this engine; this module implements the part of the HDF5 file format those files use
(HDF5 File Format Specification, version 1.x structures):

  * superblock versions 0 / 1 (and 2 / 3 as far as locating the root group's object header)
  * version-1 object headers with continuation blocks; version-2 ("OHDR") headers
  * old-style groups: symbol-table message -> version-1 B-tree ("TREE", node type 0) + local heap ("HEAP") +
    symbol-table nodes ("SNOD"); new-style groups with compact link messages
  * datasets: dataspace (versions 1, 2), fixed-point / floating-point datatypes, data layout message
    version 3 (compact, contiguous, chunked through a version-1 chunk B-tree) and versions 1 / 2
  * filters: deflate (zlib) and byte shuffle
  * attribute messages (versions 1 - 3, compact storage) on groups and datasets, as `.attrs`: fixed-point,
    floating-point, fixed-length and variable-length (global heap) string values, scalar or 1-D — what
    FAST5 readers need (the reference's network.py:199-217 reads `read_id`, `duration`, `digitisation`, ...)
Anything else raises Hdf5Error with the name of the unsupported feature."""
import struct
import zlib

import numpy as np

__all__ = ["Hdf5Error", "File", "Attributes"]

_SIG = b"\x89HDF\r\n\x1a\n"
_UNDEF = 0xFFFFFFFFFFFFFFFF


class Hdf5Error(Exception):
    pass


class _Obj:
    """an object header's messages: list of (type, flags, bytes)"""

    def __init__(self, f, addr):
        self.f = f
        self.addr = addr
        self.msgs = []
        b = f.buf
        if b[addr:addr + 4] == b"OHDR":
            self._parse_v2(addr)
        else:
            self._parse_v1(addr)

    def _parse_v1(self, addr):
        b = self.f.buf
        ver, _, nmsg, _refc, hsize = struct.unpack_from("<BBHII", b, addr)
        if ver != 1:
            raise Hdf5Error("object header version %d" % ver)
        blocks = [(addr + 16, hsize)]
        while blocks and len(self.msgs) < nmsg:
            pos, size = blocks.pop(0)
            end = pos + size
            while pos + 8 <= end and len(self.msgs) < nmsg:
                mtype, msize, mflags = struct.unpack_from("<HHB", b, pos)
                data = b[pos + 8:pos + 8 + msize]
                pos += 8 + msize
                if mtype == 0x0010:   # continuation
                    off, ln = struct.unpack_from("<QQ", data, 0)
                    blocks.append((off + self.f.base, ln))
                self.msgs.append((mtype, mflags, data))

    def _parse_v2(self, addr):
        b = self.f.buf
        ver, flags = struct.unpack_from("<BB", b, addr + 4)
        if ver != 2:
            raise Hdf5Error("OHDR version %d" % ver)
        pos = addr + 6
        if flags & 0x20:
            pos += 16
        if flags & 0x10:
            pos += 4
        csz = 1 << (flags & 3)
        size0 = int.from_bytes(b[pos:pos + csz], "little")
        pos += csz
        blocks = [(pos, size0)]
        track = bool(flags & 0x04)
        while blocks:
            pos, size = blocks.pop(0)
            end = pos + size
            while pos + 4 + (2 if track else 0) <= end:
                mtype, msize, mflags = struct.unpack_from("<BHB", b, pos)
                pos += 4 + (2 if track else 0)
                data = b[pos:pos + msize]
                pos += msize
                if mtype == 0x10:
                    off, ln = struct.unpack_from("<QQ", data, 0)
                    blocks.append((off + self.f.base + 4, ln - 8))   # skip "OCHK", drop the checksum
                self.msgs.append((mtype, mflags, data))

    def find(self, mtype):
        return [m for m in self.msgs if m[0] == mtype]


class Dataset:
    def __init__(self, f, obj, name):
        self.f, self.obj, self.name = f, obj, name
        ds = obj.find(0x0001)
        dt = obj.find(0x0003)
        lay = obj.find(0x0008)
        if not ds or not dt or not lay:
            raise Hdf5Error("%s is not a dataset" % name)
        self.shape = self._dataspace(ds[0][2])
        self.dtype = self._datatype(dt[0][2])
        self._layout = lay[0][2]
        self._filters = self._pipeline(obj.find(0x000B)[0][2]) if obj.find(0x000B) else []

    @property
    def attrs(self):
        return Attributes(self.f, self.obj, self.name)

    @staticmethod
    def _dataspace(d):
        ver, rank, flags = d[0], d[1], d[2]
        if ver == 1:
            off = 8
        elif ver == 2:
            off = 4
        else:
            raise Hdf5Error("dataspace version %d" % ver)
        return tuple(struct.unpack_from("<Q", d, off + 8 * i)[0] for i in range(rank))

    @staticmethod
    def _datatype(d):
        cls, ver = d[0] & 0x0F, d[0] >> 4
        bits0 = d[1]
        size = struct.unpack_from("<I", d, 4)[0]
        order = ">" if (bits0 & 1) else "<"
        if cls == 0:     # fixed point
            signed = bool(bits0 & 0x08)
            return np.dtype("%s%s%d" % (order if size > 1 else "|", "i" if signed else "u", size))
        if cls == 1:     # floating point
            return np.dtype("%sf%d" % (order, size))
        if cls == 3:     # fixed-length string
            return np.dtype("S%d" % size)
        raise Hdf5Error("datatype class %d" % cls)

    @staticmethod
    def _pipeline(d):
        ver, nf = d[0], d[1]
        pos = 8 if ver == 1 else 2
        out = []
        for _ in range(nf):
            fid, = struct.unpack_from("<H", d, pos)
            pos += 2
            nlen = 0
            if ver == 1 or fid >= 256:
                nlen, = struct.unpack_from("<H", d, pos)
                pos += 2
            _flags, ncd = struct.unpack_from("<HH", d, pos)
            pos += 4
            if nlen:
                pos += (nlen + 7) // 8 * 8 if ver == 1 else nlen
            cd = struct.unpack_from("<%dI" % ncd, d, pos)
            pos += 4 * ncd
            if ver == 1 and ncd % 2:
                pos += 4
            out.append((fid, cd))
        return out

    def _defilter(self, raw, mask, esize):
        for k in range(len(self._filters) - 1, -1, -1):
            if mask & (1 << k):
                continue
            fid, _cd = self._filters[k]
            if fid == 1:
                raw = zlib.decompress(raw)
            elif fid == 2:      # shuffle: bytes of all elements grouped by significance
                n = len(raw) // esize
                a = np.frombuffer(raw[:n * esize], dtype=np.uint8).reshape(esize, n).T
                raw = a.tobytes() + raw[n * esize:]
            elif fid == 3:      # fletcher32: checksum at the end
                raw = raw[:-4]
            else:
                raise Hdf5Error("filter %d" % fid)
        return raw

    def read(self):
        d = self._layout
        b = self.f.buf
        ver = d[0]
        es = self.dtype.itemsize
        n = int(np.prod(self.shape)) if self.shape else 1
        if ver == 3:
            cls = d[1]
            if cls == 0:
                size, = struct.unpack_from("<H", d, 2)
                return np.frombuffer(d[4:4 + size], dtype=self.dtype, count=n).reshape(self.shape).copy()
            if cls == 1:
                addr, size = struct.unpack_from("<QQ", d, 2)
                if addr == _UNDEF:
                    return np.zeros(self.shape, dtype=self.dtype)
                return np.frombuffer(b, dtype=self.dtype, count=n, offset=addr + self.f.base).reshape(self.shape).copy()
            if cls == 2:
                nd = d[2]
                bt, = struct.unpack_from("<Q", d, 3)
                cdims = struct.unpack_from("<%dI" % nd, d, 11)
                return self._read_chunked(bt, cdims[:-1], nd)
            raise Hdf5Error("layout class %d" % cls)
        if ver in (1, 2):
            nd, cls = d[1], d[2]
            pos = 8
            addr = None
            if cls != 0:
                addr, = struct.unpack_from("<Q", d, pos)
                pos += 8
            dims = struct.unpack_from("<%dI" % nd, d, pos)
            if cls == 1:
                return np.frombuffer(b, dtype=self.dtype, count=n, offset=addr + self.f.base).reshape(self.shape).copy()
            if cls == 2:
                return self._read_chunked(addr, dims[:-1], nd)
            raise Hdf5Error("layout class %d (message version %d)" % (cls, ver))
        raise Hdf5Error("data layout message version %d" % ver)

    def _read_chunked(self, btree, cdims, nd):
        out = np.zeros(self.shape, dtype=self.dtype)
        if btree == _UNDEF:
            return out
        es = self.dtype.itemsize
        rank = len(self.shape)
        if len(cdims) != rank:
            raise Hdf5Error("chunk rank %d for a rank-%d dataset" % (len(cdims), rank))
        stack = [btree + self.f.base]
        b = self.f.buf
        while stack:
            addr = stack.pop()
            if b[addr:addr + 4] != b"TREE":
                raise Hdf5Error("chunk index is not a version-1 B-tree")
            ntype, level, used = struct.unpack_from("<BBH", b, addr + 4)
            if ntype != 1:
                raise Hdf5Error("B-tree node type %d in a chunk index" % ntype)
            pos = addr + 8 + 16
            ksz = 8 + 8 * nd
            for _ in range(used):
                csize, mask = struct.unpack_from("<II", b, pos)
                offs = struct.unpack_from("<%dQ" % nd, b, pos + 8)
                child, = struct.unpack_from("<Q", b, pos + ksz)
                pos += ksz + 8
                if level > 0:
                    stack.append(child + self.f.base)
                    continue
                raw = self._defilter(bytes(b[child + self.f.base:child + self.f.base + csize]), mask, es)
                want = int(np.prod(cdims)) * es
                if len(raw) < want:      # a clipped edge chunk (some writers store only the rows that exist)
                    raw = raw + b"\0" * (want - len(raw))
                chunk = np.frombuffer(raw, dtype=self.dtype, count=int(np.prod(cdims))).reshape(cdims)
                sl_out, sl_in = [], []
                for dmn in range(rank):
                    lo = offs[dmn]
                    hi = min(lo + cdims[dmn], self.shape[dmn])
                    sl_out.append(slice(lo, hi))
                    sl_in.append(slice(0, hi - lo))
                out[tuple(sl_out)] = chunk[tuple(sl_in)]
        return out

    def __array__(self, dtype=None, copy=None):
        a = self.read()
        return a.astype(dtype) if dtype is not None else a


def _pad8(n):
    return (n + 7) // 8 * 8


class Attributes:
    """An object's attribute messages (0x000C), read-only and dict-like, with h5py's value conventions: a scalar
    attribute is a NumPy scalar (fixed-length strings: bytes), a 1-D one an array; variable-length strings are str.
    Attributes kept in dense storage (an attribute-info message with a fractal heap) raise Hdf5Error."""

    def __init__(self, f, obj, name):
        self.f, self.name = f, name
        self._raw = {}
        for _t, _fl, d in obj.find(0x000C):
            nm, dt, ds, data = self._split(d)
            self._raw[nm] = (dt, ds, data)
        if not self._raw:
            for _t, _fl, d in obj.find(0x0015):     # attribute info: dense storage unless its heap address is undefined
                pos = 2 + (2 if d[1] & 1 else 0)
                fh, = struct.unpack_from("<Q", d, pos)
                if fh != _UNDEF:
                    raise Hdf5Error("dense attribute storage (fractal heap) in %s" % name)

    @staticmethod
    def _split(d):
        ver = d[0]
        nsz, tsz, ssz = struct.unpack_from("<HHH", d, 2)
        if ver == 1:
            pos = 8
            nm = bytes(d[pos:pos + nsz]); pos += _pad8(nsz)
            dt = bytes(d[pos:pos + tsz]); pos += _pad8(tsz)
            ds = bytes(d[pos:pos + ssz]); pos += _pad8(ssz)
        elif ver in (2, 3):
            pos = 8 if ver == 2 else 9
            nm = bytes(d[pos:pos + nsz]); pos += nsz
            dt = bytes(d[pos:pos + tsz]); pos += tsz
            ds = bytes(d[pos:pos + ssz]); pos += ssz
        else:
            raise Hdf5Error("attribute message version %d" % ver)
        return nm.rstrip(b"\0").decode(), dt, ds, bytes(d[pos:])

    def keys(self):
        return list(self._raw)

    def __iter__(self):
        return iter(self.keys())

    def __len__(self):
        return len(self._raw)

    def __contains__(self, k):
        return k in self._raw

    def items(self):
        return [(k, self[k]) for k in self._raw]

    def get(self, k, default=None):
        return self[k] if k in self._raw else default

    def __getitem__(self, k):
        if k not in self._raw:
            raise KeyError("%s has no attribute %r" % (self.name, k))
        dt, ds, data = self._raw[k]
        if ds[0] == 2 and ds[3] == 2:       # null dataspace
            return None
        shape = Dataset._dataspace(ds)
        if len(shape) > 1:
            raise Hdf5Error("attribute %r of rank %d" % (k, len(shape)))
        n = int(np.prod(shape)) if shape else 1
        cls = dt[0] & 0x0F
        if cls == 9:                        # variable-length
            if (dt[1] & 0x0F) != 1:
                raise Hdf5Error("variable-length sequence attribute %r" % k)
            vals = [self._vlen_string(data, 16 * i) for i in range(n)]
            return vals[0] if not shape else np.array(vals, dtype=object)
        dtype = Dataset._datatype(dt)
        a = np.frombuffer(data, dtype=dtype, count=n)     # (fixed-length strings: bytes, NULs stripped, as h5py)
        return a[0] if not shape else a.reshape(shape).copy()

    def _vlen_string(self, data, pos):
        ln, addr, idx = struct.unpack_from("<IQI", data, pos)
        if ln == 0 or addr == 0 or addr == _UNDEF:
            return ""
        b = self.f.buf
        col = addr + self.f.base
        if b[col:col + 4] != b"GCOL":
            raise Hdf5Error("global heap signature")
        csize, = struct.unpack_from("<Q", b, col + 8)
        p, end = col + 16, col + csize
        while p + 16 <= end:
            oidx, _ref, osize = struct.unpack_from("<HH4xQ", b, p)
            if oidx == 0:
                break
            if oidx == idx:
                return bytes(b[p + 16:p + 16 + min(ln, osize)]).decode("utf-8")
            p += 16 + _pad8(osize)
        raise Hdf5Error("global heap object %d not found" % idx)


class Group:
    def __init__(self, f, obj, name):
        self.f, self.obj, self.name = f, obj, name
        self._links = None

    @property
    def attrs(self):
        return Attributes(self.f, self.obj, self.name)

    def _load(self):
        if self._links is not None:
            return
        links = {}
        b = self.f.buf
        for _t, _fl, d in self.obj.find(0x0011):      # symbol table: B-tree + local heap
            bt, heap = struct.unpack_from("<QQ", d, 0)
            heap += self.f.base
            if b[heap:heap + 4] != b"HEAP":
                raise Hdf5Error("local heap signature")
            dseg, = struct.unpack_from("<Q", b, heap + 24)
            dseg += self.f.base
            stack = [bt + self.f.base]
            while stack:
                addr = stack.pop()
                if b[addr:addr + 4] == b"TREE":
                    ntype, level, used = struct.unpack_from("<BBH", b, addr + 4)
                    pos = addr + 8 + 16
                    children = []
                    for i in range(used):
                        child, = struct.unpack_from("<Q", b, pos + 8)       # key (8) then child (8)
                        children.append(child + self.f.base)
                        pos += 16
                    stack.extend(reversed(children))
                elif b[addr:addr + 4] == b"SNOD":
                    nsym, = struct.unpack_from("<H", b, addr + 6)
                    pos = addr + 8
                    for _ in range(nsym):
                        noff, oaddr = struct.unpack_from("<QQ", b, pos)
                        end = b.index(b"\0", dseg + noff)
                        links[b[dseg + noff:end].decode()] = oaddr + self.f.base
                        pos += 40
                else:
                    raise Hdf5Error("group B-tree node signature %r" % bytes(b[addr:addr + 4]))
        for _t, _fl, d in self.obj.find(0x0006):      # link message (new-style compact groups)
            ver, flags = d[0], d[1]
            pos = 2
            ltype = 0
            if flags & 0x08:
                ltype = d[pos]; pos += 1
            if flags & 0x04:
                pos += 8
            if flags & 0x10:
                pos += 1
            lsz = 1 << (flags & 3)
            nlen = int.from_bytes(d[pos:pos + lsz], "little"); pos += lsz
            nm = bytes(d[pos:pos + nlen]).decode(); pos += nlen
            if ltype == 0:
                links[nm] = struct.unpack_from("<Q", d, pos)[0] + self.f.base
        if self.obj.find(0x0002) and not links:
            info = self.obj.find(0x0002)[0][2]
            fh, = struct.unpack_from("<Q", info, 2)
            if fh != _UNDEF:
                raise Hdf5Error("dense link storage (fractal heap)")
        self._links = links

    def keys(self):
        self._load()
        return sorted(self._links)       # h5py iterates old-style groups in name order

    def __iter__(self):
        return iter(self.keys())

    def __contains__(self, k):
        self._load()
        return k in self._links

    def __getitem__(self, path):
        node = self.f if path.startswith("/") else self
        for part in [p for p in path.split("/") if p]:
            if not isinstance(node, Group):
                raise KeyError(path)
            node._load()
            if part not in node._links:
                raise KeyError("%s (no %r in %s)" % (path, part, node.name))
            node = node.f._open(node._links[part], (node.name.rstrip("/") + "/" + part))
        return node


class File(Group):
    def __init__(self, path, mode="r"):
        if mode != "r":
            raise Hdf5Error("read-only")
        with open(path, "rb") as fh:
            self.buf = fh.read()
        self.base = 0
        b = self.buf
        pos = 0
        while b[pos:pos + 8] != _SIG:      # the superblock may sit at 0, 512, 1024, ...
            pos = 512 if pos == 0 else pos * 2
            if pos + 8 > len(b):
                raise Hdf5Error("not an HDF5 file")
        ver = b[pos + 8]
        if ver in (0, 1):
            so, sl = b[pos + 13], b[pos + 14]
            if so != 8 or sl != 8:
                raise Hdf5Error("offset / length size %d / %d" % (so, sl))
            p = pos + 24 + (4 if ver == 1 else 0)
            self.base, = struct.unpack_from("<Q", b, p)
            root_ste = p + 32
            root_addr, = struct.unpack_from("<Q", b, root_ste + 8)
        elif ver in (2, 3):
            if b[pos + 9] != 8 or b[pos + 10] != 8:
                raise Hdf5Error("offset / length size")
            self.base, = struct.unpack_from("<Q", b, pos + 12)
            root_addr, = struct.unpack_from("<Q", b, pos + 36)
        else:
            raise Hdf5Error("superblock version %d" % ver)
        self._cache = {}
        Group.__init__(self, self, _Obj(self, root_addr + self.base), "/")

    def _open(self, addr, name):
        if addr not in self._cache:
            obj = _Obj(self, addr)
            self._cache[addr] = Dataset(self, obj, name) if obj.find(0x0008) else Group(self, obj, name)
        return self._cache[addr]

    def close(self):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False
