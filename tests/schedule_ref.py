"""Host-side model of a two-stream launch list (hd_yolo_amd/plan.py's backward list, hd_yolo_amd/ops.py's SideStream, csrc/exec.hip).

A list is a sequence of launch records `(symbol, args, kept tensors[, host arrays])` on the main stream, `('@fork', side, [records], token)`
records whose launches go to the side stream once everything issued so far on the main stream is done, `('@join', side, token)` records at
which the main stream waits for the fork that carries `token` (side-stream work is in order: for every fork at or before that one in the
list too), and `('@call', fn)` host callbacks.  Nothing here launches a kernel; plain Python and torch (CPU tensors have data_ptr() too).

  windows(recs)     for every fork: the main-stream records that may run beside it, plus the structural rules of a list
  footprint(rec)    the bytes every pointer argument of a launch record covers, and whether the launch may write them
  conflicts(recs)   every (forked record, main record in its window) pair whose footprints overlap with one side writable: a data race
  canonical(recs)   the list with addresses replaced by (storage ordinal, offset, shape of the region): equal for equal lists over other memory
  writers(...)      launch records that may write a byte range, from a list position on (the "gradient range is final" marks)
  early / late      the two extreme legal orders of a list, run on ONE stream: a missing join makes them compute different numbers

Which pointers are written comes from the prototypes of include/hdyolo.h (`const T*` is read, any other pointer may be written), how far
they reach from the tensors a record keeps alive (matched by data_ptr()), NHWC channel slices as rows at a pitch.
"""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'hdyolo.h')


class ScheduleError(AssertionError):
    """the list itself is malformed, or the checker cannot account for one of its arguments (never skipped silently)"""


# ------------------------------------------------------------------------------------------ prototypes (include/hdyolo.h)
class Param:
    __slots__ = ('name', 'pointer', 'const', 'ctype')

    def __init__(self, name, pointer, const, ctype):
        self.name, self.pointer, self.const, self.ctype = name, pointer, const, ctype

    def __repr__(self):
        return f'{self.ctype} {self.name}'


_protos = {}


def prototypes(path=HEADER):
    """{symbol: [Param]} of every function include/hdyolo.h declares (tests/test_abi.py's way of reading it: comments out, one regex)"""
    if path not in _protos:
        text = re.sub(r'/\*.*?\*/', '', open(path).read(), flags=re.S)
        text = re.sub(r'//[^\n]*', '', text)
        out = {}
        for name, params in re.findall(r'\b(hdy_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;', text, flags=re.S):
            plist = []
            for p in (q.strip() for q in params.split(',')):
                if p in ('', 'void'):
                    continue
                m = re.match(r'^(.*?)(\w+)\s*(\[\s*\])?$', ' '.join(p.split()), flags=re.S)
                if m is None or not m.group(1).strip():
                    raise ScheduleError(f'{name}: cannot read parameter {p!r}')
                ctype = m.group(1).strip() + ('*' if m.group(3) else '')
                plist.append(Param(m.group(2), '*' in ctype, re.match(r'^const\b', ctype) is not None, ctype))
            out[name] = plist
        _protos[path] = out
    return _protos[path]


def return_types(path=HEADER):
    """{symbol: the text of its return type}, read the same way: a prototype starts its line with the return type"""
    text = re.sub(r'/\*.*?\*/', '', open(path).read(), flags=re.S)
    text = re.sub(r'//[^\n]*', '', text)
    return {name: ' '.join(ret.split()) for ret, name in re.findall(r'^((?:const )?[a-z_ ]+?\**)\s*\b(hdy_[a-z0-9_]+)\s*\(', text, flags=re.M)}


def record(symbol, **kw):
    """A hand-made launch record of `symbol`: parameters by the header's names, tensors for pointers (kept by the record, as ops._rec does),
    everything not named 0 / NULL.  The trailing stream is not part of a record."""
    params = prototypes()[symbol]
    assert params and params[-1].name == 'stream', symbol
    unknown = set(kw) - {p.name for p in params[:-1]}
    if unknown:
        raise ScheduleError(f'{symbol} has no parameter(s) {sorted(unknown)}')
    args, keep = [], []
    for p in params[:-1]:
        v = kw.get(p.name, None if p.pointer else 0)
        if hasattr(v, 'data_ptr'):
            keep.append(v)
            v = v.data_ptr()
        args.append(v)
    return (symbol, tuple(args), tuple(keep))


# ------------------------------------------------------------------------------------------ byte regions
class Region:
    """`rows` runs of `row` bytes, `pitch` bytes apart, from address `base` (rows == 1: one plain range)"""
    __slots__ = ('base', 'rows', 'row', 'pitch')

    def __init__(self, base, rows, row, pitch=None):
        self.base, self.rows, self.row = int(base), int(rows), int(row)
        self.pitch = int(row if pitch is None or rows == 1 else pitch)
        assert self.rows >= 1 and self.row >= 0 and (self.rows == 1 or self.pitch >= self.row), (rows, row, pitch)

    lo = property(lambda self: self.base)
    hi = property(lambda self: self.base + (self.rows - 1) * self.pitch + self.row)

    def __eq__(self, o):
        return (self.base, self.rows, self.row, self.pitch) == (o.base, o.rows, o.row, o.pitch)

    def __hash__(self):
        return hash((self.base, self.rows, self.row, self.pitch))

    def __repr__(self):
        if self.rows == 1:
            return f'[{self.base:#x}, +{self.row})'
        return f'[{self.base:#x}: {self.rows} rows of {self.row} bytes at pitch {self.pitch}]'

    def inside(self, t):
        """does the region lie within tensor t's own span of bytes?"""
        s = region_of(t)
        return s.lo <= self.lo and self.hi <= s.hi


def region_of(t, base=None):
    """The bytes a tensor view really covers.  A view whose innermost dimensions are dense and whose outer dimensions step uniformly (an NHWC
    channel slice `buf[..., k0:k0 + K]`, a `[:, :, k0:]` slice of statistics slabs) is rows at a pitch; anything else the plain range from its
    first to its last element."""
    es = t.element_size()
    p = t.data_ptr() if base is None else base
    if t.numel() == 0:
        return Region(p, 1, 0)
    dims = [(s, st) for s, st in zip(t.shape, t.stride()) if s > 1]
    span = (sum((s - 1) * abs(st) for s, st in dims) + 1) * es
    if any(st <= 0 for _, st in dims):
        return Region(p, 1, span)
    run, i = 1, len(dims) - 1
    while i >= 0 and dims[i][1] == run:
        run *= dims[i][0]
        i -= 1
    if i < 0:
        return Region(p, 1, run * es)
    pitch, rows = dims[i][1], dims[i][0]
    uniform = pitch >= run
    for j in range(i - 1, -1, -1):
        uniform = uniform and dims[j][1] == dims[j + 1][0] * dims[j + 1][1]
        rows *= dims[j][0]
    if not uniform:
        return Region(p, 1, span)
    return Region(p, rows, run * es, pitch * es)


def overlap(a, b):
    """Do two regions share a byte?  Exact for two plain ranges, for rows of ONE pitch (two channel slices of one buffer overlap only if their
    column ranges do) and for a short plain range against rows; conservative (the bounding ranges) for everything else."""
    if a.row == 0 or b.row == 0 or a.hi <= b.lo or b.hi <= a.lo:
        return False
    if a.rows == 1 and b.rows == 1:
        return True
    if a.rows > 1 and b.rows > 1 and a.pitch != b.pitch:
        return True
    P = a.pitch if a.rows > 1 else b.pitch
    if (a.rows == 1 and a.row > P) or (b.rows == 1 and b.row > P):
        return True
    # row i of a against row j of b, seen from a.base - j * P: [k * P, k * P + a.row) against [d, d + b.row) with k = i - j
    d = b.base - a.base
    for k in (d // P - 1, d // P, d // P + 1):
        if -(b.rows - 1) <= k <= a.rows - 1 and k * P < d + b.row and d < k * P + a.row:
            return True
    return False


# ------------------------------------------------------------------------------------------ footprints
class Access:
    __slots__ = ('arg', 'write', 'region')

    def __init__(self, arg, write, region):
        self.arg, self.write, self.region = arg, write, region

    def __repr__(self):
        return f"{'write' if self.write else 'read'} {self.arg} {self.region}"


def _addr(v):
    if v is None:
        return 0
    if isinstance(v, int):
        return v
    if isinstance(v, ctypes._SimpleCData):
        return v.value or 0
    return ctypes.cast(v, ctypes.c_void_p).value or 0


def _extent(p, keep, what):
    """region behind pointer `p`: the kept tensor that starts there (several: they must agree, else the widest plain range); failing that a
    kept tensor that CONTAINS it (an interior pointer such as hdy_bn_finalize_sums' `sums + k0`): from p to that tensor's end"""
    exact = {region_of(t) for t in keep if t.data_ptr() == p}
    if len(exact) == 1:
        return next(iter(exact))
    if exact:
        return Region(p, 1, max(r.hi for r in exact) - p)
    inner = [region_of(t) for t in keep if t.data_ptr() < p < region_of(t).hi]
    if inner:
        return Region(p, 1, max(r.hi for r in inner) - p)
    raise ScheduleError(f'{what} = {p:#x}: no tensor kept by the record starts at or spans this address: its extent is unknown')


def footprint(rec):
    """[Access] of a launch record: one entry per non-null pointer argument (the hdy_stat_req array of the *_stats entry points: four per
    request — `slabs` written, `y` / `scale` / `shift` read, as ops.StatRequest.keep lists them)."""
    name, args = rec[0], rec[1]
    if name[0] == '@':
        raise ScheduleError(f'{name} is not a launch record')
    params = prototypes().get(name)
    if params is None:
        raise ScheduleError(f'{name} is not declared in include/hdyolo.h')
    if not params or params[-1].name != 'stream' or len(args) != len(params) - 1:
        raise ScheduleError(f'{name}: {len(args)} arguments recorded, the prototype takes {len(params) - 1} in front of the stream')
    keep = [t for t in rec[2] if hasattr(t, 'data_ptr')]
    out = []
    for n, (p, v) in enumerate(zip(params, args)):
        if not p.pointer:
            continue
        a = _addr(v)
        if a == 0:
            continue
        if 'hdy_stat_req' in p.ctype:
            arrs = [x for x in (rec[3] if len(rec) > 3 else ()) if ctypes.addressof(x) == a]
            if not arrs:
                raise ScheduleError(f'{name}[{p.name}]: the record does not keep the request array at {a:#x}')
            nreq = args[n + 1]
            assert params[n + 1].name == 'nstat' and nreq == len(arrs[0]), (name, nreq, len(arrs[0]))
            for i, q in enumerate(arrs[0]):
                for f, write in (('y', False), ('scale', False), ('shift', False), ('slabs', True)):
                    fa = getattr(q, f) or 0
                    if fa:
                        out.append(Access(f'{p.name}[{i}].{f}', write, _extent(fa, keep, f'{name}[{p.name}[{i}].{f}]')))
            continue
        out.append(Access(p.name, not p.const, _extent(a, keep, f'{name}[{p.name}]')))
    return out


# ------------------------------------------------------------------------------------------ canonical form
STAT_REQ_POINTERS = ('y', 'scale', 'shift', 'slabs')


def canonical(recs):
    """The list with the addresses taken out, for comparing two lists built over different allocations: per record the symbol and its
    arguments, scalars verbatim, a null pointer as None, every other pointer as (ordinal of its underlying storage in order of first
    appearance in the list, byte offset inside that storage, rows, row bytes, pitch of the region behind it).  An hdy_stat_req array becomes
    its requests field by field; '@fork' keeps its token and the canonical form of its records, '@join' its token, '@call' the range of its
    `hdy_mark` or the tag 'host'.  A pointer no kept tensor accounts for raises ScheduleError, as in footprint()."""
    ordinal = {}

    def pointer(p, keep, what):
        r = _extent(p, keep, what)
        bases = {t.untyped_storage().data_ptr() for t in keep if t.data_ptr() <= p < max(region_of(t).hi, t.data_ptr() + 1)}
        if len(bases) != 1:
            raise ScheduleError(f'{what} = {p:#x}: the tensors kept there belong to {len(bases)} storages')
        base = bases.pop()
        return (ordinal.setdefault(base, len(ordinal)), p - base, r.rows, r.row, r.pitch)

    def launch(rec):
        name, args = rec[0], rec[1]
        footprint(rec)                          # the structural checks: declared, argument count, request array kept
        keep = [t for t in rec[2] if hasattr(t, 'data_ptr')]
        out = []
        for p, v in zip(prototypes()[name], args):
            if not p.pointer:
                out.append(v.value if isinstance(v, ctypes._SimpleCData) else v)
            elif _addr(v) == 0:
                out.append(None)
            elif 'hdy_stat_req' in p.ctype:
                arr = next(x for x in rec[3] if ctypes.addressof(x) == _addr(v))
                out.append(tuple(tuple(pointer(getattr(q, f), keep, f'{name}[{p.name}[{i}].{f}]') if f in STAT_REQ_POINTERS and getattr(q, f) else
                                       getattr(q, f) for f, _ in q._fields_) for i, q in enumerate(arr)))
            else:
                out.append(pointer(_addr(v), keep, f'{name}[{p.name}]'))
        return (name, tuple(out))

    out = []
    for r in recs:
        if r[0] == '@fork':
            out.append(('@fork', r[3], tuple(launch(q) for q in r[2])))
        elif r[0] == '@join':
            out.append(('@join', r[2]))
        elif r[0] == '@call':
            out.append(('@call', tuple(r[1].hdy_mark) if hasattr(r[1], 'hdy_mark') else 'host'))
        else:
            out.append(launch(r))
    return out


# ------------------------------------------------------------------------------------------ list structure
def windows(recs):
    """{position of a fork: [positions of the records the main stream may run beside it]}: everything behind the fork and in front of the
    first join that covers it (forks and joins themselves left out; '@call' records are part of the main sequence and listed).  A join of
    token t covers the fork that carries t and, the side stream being in order, every fork at an earlier list position — tokens are NOT
    monotonic in list order, positions are.  Raises ScheduleError for a token carried twice, a join whose token no earlier fork carries,
    and a fork that no join covers before the list ends."""
    where = {}
    for i, r in enumerate(recs):
        if r[0] == '@fork':
            if r[3] in where:
                raise ScheduleError(f'forks at {where[r[3]]} and {i} carry the same token {r[3]}')
            where[r[3]] = i
    joins = []
    for j, r in enumerate(recs):
        if r[0] == '@join':
            if r[2] not in where or where[r[2]] > j:
                raise ScheduleError(f"'@join' at {j} names token {r[2]}, which no fork in front of it carries")
            joins.append((j, where[r[2]]))
    out = {}
    for i, r in enumerate(recs):
        if r[0] != '@fork':
            continue
        end = next((j for j, f in joins if j > i and f >= i), None)
        if end is None:
            raise ScheduleError(f"'@fork' at {i} (token {r[3]}, {[q[0] for q in r[2]]}) is not covered by any '@join' before the list ends")
        out[i] = [k for k in range(i + 1, end) if recs[k][0] not in ('@fork', '@join')]
    return out


class Conflict:
    __slots__ = ('fork_pos', 'fork_symbol', 'fork_arg', 'fork_write', 'fork_region', 'main_pos', 'main_symbol', 'main_arg', 'main_write', 'main_region')

    def __init__(self, *v):
        for k, x in zip(self.__slots__, v):
            setattr(self, k, x)

    def __repr__(self):
        w = lambda f: 'writes' if f else 'reads'
        return (f"{self.fork_symbol} forked at {self.fork_pos} {w(self.fork_write)} `{self.fork_arg}` {self.fork_region} while {self.main_symbol} at "
                f"{self.main_pos} (main stream) {w(self.main_write)} `{self.main_arg}` {self.main_region}: no '@join' between {self.fork_pos} and "
                f"{self.main_pos} covers the fork")


def conflicts(recs):
    """[Conflict]: every pair (record of a fork, main-stream launch record in the fork's window) with overlapping footprints of which at least one
    may write.  Host callbacks have no footprint here."""
    fp = {}

    def of(key, rec):
        if key not in fp:
            acc = footprint(rec)
            fp[key] = (acc, min([a.region.lo for a in acc] + [1 << 63]), max([a.region.hi for a in acc] + [0]))
        return fp[key]

    out = []
    for i, win in windows(recs).items():
        for n, frec in enumerate(recs[i][2]):
            facc, flo, fhi = of((i, n), frec)
            for j in win:
                if recs[j][0][0] == '@':
                    continue
                macc, mlo, mhi = of(j, recs[j])
                if mhi <= flo or fhi <= mlo:
                    continue
                for a in facc:
                    for b in macc:
                        if (a.write or b.write) and overlap(a.region, b.region):
                            out.append(Conflict(i, frec[0], a.arg, a.write, a.region, j, recs[j][0], b.arg, b.write, b.region))
    return out


def launches(recs, start=0):
    """(position, record) of every launch record at or behind list position `start`, fork bodies included"""
    for i in range(start, len(recs)):
        r = recs[i]
        if r[0] == '@fork':
            for q in r[2]:
                yield i, q
        elif r[0][0] != '@':
            yield i, r


def writers(recs, lo, hi, start=0):
    """[(position, symbol, argument)] of the launch records at or behind `start` that may write a byte of [lo, hi)"""
    target = Region(lo, 1, hi - lo)
    return [(i, r[0], a.arg) for i, r in launches(recs, start) for a in footprint(r) if a.write and overlap(a.region, target)]


def early_marks(recs, flat):
    """the '@call' marks "elements [a, b) of `flat` (the fp32 gradient store) are final" (Plan._mark_buckets) that come too early:
    [(mark position, (a, b), later writers)].  Derived from the footprints alone, not from the plan's own log."""
    bad = []
    base = flat.data_ptr()
    for i, r in enumerate(recs):
        if r[0] == '@call' and hasattr(r[1], 'hdy_mark'):
            a, b = r[1].hdy_mark
            late_writers = writers(recs, base + 4 * a, base + 4 * b, start=i)
            if late_writers:
                bad.append((i, (a, b), late_writers))
    return bad


# ------------------------------------------------------------------------------------------ the two extreme legal orders, on one stream
class _Order:
    """Takes the place of a SideStream's fork / join (instance attributes, restored on exit) while a list runs through ops.run."""

    def __init__(self, side, run=None):
        self.side, self._run = side, run

    def run(self, records):
        if self._run is None:
            from hd_yolo_amd import ops
            self._run = ops.run
        self._run(records)          # on the current stream: the one the main list runs on

    def __enter__(self):
        self._saved = {k: self.side.__dict__.get(k) for k in ('fork', 'join')}
        self.side.fork, self.side.join = self.fork, self.join
        return self

    def __exit__(self, *exc):
        for k, v in self._saved.items():
            if v is None:
                self.side.__dict__.pop(k, None)
            else:
                setattr(self.side, k, v)
        if exc[0] is None:
            self.finish()
        return False

    def finish(self):
        pass


class early(_Order):
    """The earliest legal order: a fork's records run at the fork point, a join has nothing to wait for."""

    def fork(self, records, token, main):
        self.run(records)

    def join(self, token, main):
        pass


class late(_Order):
    """The latest legal order: forks queue up and run, in order, at the first join that covers them.  plan: a '@call' mark of that plan
    whose bucket hook is installed flushes the queue too (the hook's consumer waits for the side stream before it reads the range)."""

    def __init__(self, side, plan=None, run=None):
        super().__init__(side, run)
        self.queue, self.plan = [], plan

    def fork(self, records, token, main):
        self.queue.append((token, records))

    def join(self, token, main):
        at = next((i for i, (t, _) in enumerate(self.queue) if t == token), None)
        if at is not None:                  # (None: flushed before, or never forked — as SideStream.join, nothing to wait for)
            self.flush(at + 1)

    def flush(self, n=None):
        todo, self.queue = self.queue[:n], self.queue[len(self.queue) if n is None else n:]
        for _, records in todo:
            self.run(records)

    def __enter__(self):
        super().__enter__()
        self._hook = None
        if self.plan is not None and self.plan.bucket_hook is not None:
            self._hook = hook = self.plan.bucket_hook

            def flushing(a, b, stream):
                self.flush()
                return hook(a, b, stream)
            self.plan.bucket_hook = flushing
        return self

    def __exit__(self, *exc):
        if self._hook is not None:
            self.plan.bucket_hook = self._hook
        return super().__exit__(*exc)

    def finish(self):
        if self.queue:
            raise ScheduleError(f'{len(self.queue)} fork(s) were never joined: tokens {[t for t, _ in self.queue]}')
