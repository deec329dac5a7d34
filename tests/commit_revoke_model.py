"""The specification of cordahip_commit_log_revoke and cordahip_commit_log_export, and the tools
the tests use to build their inputs.

RevokeModel extends tests/commit_log_model.py's dict with each entry's sequence number as
include/cordahip.h defines it (a loaded row carries 0; transaction t of a commit call carries
next_seq as cordahip_commit_log_stats reported it before the call, plus t -- every transaction
of a call consumes a number, whatever its outcome), with revoke -- what a rollback of the
reference's database transaction does to PersistentUniquenessProvider's JDBC-backed map
(PersistentUniquenessProvider.kt:62-82) -- and with export, the `snapshot` of
DistributedImmutableMap.kt:80-98.

hash_ref is corda_amd/csrc/commit_core.hpp's slot index in plain Python (SipHash-1-3 of the 36
ref bytes under the log's salt), and TableSim the table itself at slot level (linear probing, the
core's `put` order, backward-shift removal): a test whose case depends on where entries lie --
the first slot of a cluster, a cluster that wraps the table's end -- proves with it that its
inputs have that shape before it asks the GPU."""
import struct

from commit_log_model import CommitLogModel

M64 = (1 << 64) - 1


def _rotl(x, b):
    return ((x << b) | (x >> (64 - b))) & M64


def siphash13(data: bytes, k0: int, k1: int) -> int:
    """SipHash-1-3 (one compression round, three finalisation rounds) of `data`."""
    v0, v1 = k0 ^ 0x736f6d6570736575, k1 ^ 0x646f72616e646f6d
    v2, v3 = k0 ^ 0x6c7967656e657261, k1 ^ 0x7465646279746573

    def rnd():
        nonlocal v0, v1, v2, v3
        v0 = (v0 + v1) & M64
        v1 = _rotl(v1, 13) ^ v0
        v0 = _rotl(v0, 32)
        v2 = (v2 + v3) & M64
        v3 = _rotl(v3, 16) ^ v2
        v0 = (v0 + v3) & M64
        v3 = _rotl(v3, 21) ^ v0
        v2 = (v2 + v1) & M64
        v1 = _rotl(v1, 17) ^ v2
        v2 = _rotl(v2, 32)

    padded = data + bytes(7 - len(data) % 8) + bytes([len(data) & 0xff])
    for (m,) in struct.iter_unpack("<Q", padded):
        v3 ^= m
        rnd()
        v0 ^= m
    v2 ^= 0xff
    rnd()
    rnd()
    rnd()
    return v0 ^ v1 ^ v2 ^ v3


def ref_bytes(ref) -> bytes:
    return bytes(ref[0]) + struct.pack("<I", ref[1])


def hash_ref(ref, k0: int, k1: int) -> int:
    """commit_core.hpp's hash_ref for ref = (txhash, index)."""
    return siphash13(ref_bytes(ref), k0, k1)


def salt_keys(salt: bytes):
    """(k0, k1) as cordahip_commit_log_create reads its 16 salt bytes."""
    return struct.unpack("<QQ", salt)


class TableSim:
    """2^log2 slots, each None or a ref, filled and emptied as commit_core.hpp does it."""

    def __init__(self, log2: int, salt: bytes):
        self.n = 1 << log2
        self.k0, self.k1 = salt_keys(salt)
        self.slots = [None] * self.n

    def home(self, ref):
        return hash_ref(ref, self.k0, self.k1) & (self.n - 1)

    def slot_of(self, ref):
        s = self.home(ref)
        for _ in range(self.n):
            if self.slots[s] is None:
                return None
            if self.slots[s] == ref:
                return s
            s = (s + 1) % self.n
        return None

    def put(self, ref):
        """`put` / insert_absent: the first empty slot of the probe sequence. Returns the slot."""
        ref = (bytes(ref[0]), int(ref[1]))
        at = self.slot_of(ref)
        if at is not None:
            return at
        s = self.home(ref)
        while self.slots[s] is not None:
            s = (s + 1) % self.n
        self.slots[s] = ref
        return s

    def erase(self, ref):
        """erase_at on the ref's slot. Returns {moved ref: (from slot, to slot)}."""
        i = self.slot_of((bytes(ref[0]), int(ref[1])))
        assert i is not None
        moves, j = {}, i
        for _ in range(self.n):
            j = (j + 1) % self.n
            if self.slots[j] is None:
                break
            if (j - self.home(self.slots[j])) % self.n < (j - i) % self.n:
                continue
            self.slots[i] = self.slots[j]
            moves[self.slots[j]] = (j, i)
            i = j
        self.slots[i] = None
        return moves

    def clusters(self):
        """Maximal cyclic runs of occupied slots: [[slot, ...]] each in probe order from its first
        slot (so a run that wraps the table's end reads ..., n-1, 0, ...)."""
        out = []
        for s in range(self.n):
            if self.slots[s] is not None and self.slots[s - 1] is None:
                run = []
                while self.slots[s] is not None and len(run) < self.n:
                    run.append(s)
                    s = (s + 1) % self.n
                out.append(run)
        return out

    def cluster_of(self, ref):
        s = self.slot_of((bytes(ref[0]), int(ref[1])))
        return next(c for c in self.clusters() if s in c)

    def entries(self):
        return sum(1 for r in self.slots if r is not None)


def _key(ref):
    return (bytes(ref[0]), int(ref[1]))


def _by(by):
    return (bytes(by[0]), int(by[1]), int(by[2]))


class RevokeModel(CommitLogModel):
    def __init__(self):
        super().__init__()
        self.seq = {}       # ref -> sequence number, for exactly the keys of self.log
        self.next_seq = 1   # cordahip_commit_log_stats's next_seq
        self._now = 0

    def load(self, rows):
        before = set(self.log)
        dup = super().load(rows)
        for r in set(self.log) - before:
            self.seq[r] = 0
        return dup

    def commit_one(self, txid, caller, refs):
        res = super().commit_one(txid, caller, refs)
        if res[1]:
            for r in refs:
                self.seq[_key(r)] = self._now
        return res

    def commit_batch(self, txs, now_ns=0, tolerance_ns=0, gate=None):
        out = ([], [], [], [])
        for t, tx in enumerate(txs):
            self._now = self.next_seq + t
            one = super().commit_batch([tx], now_ns, tolerance_ns, None if gate is None else [gate[t]])
            for acc, v in zip(out, one):
                acc.extend(v)
        self.next_seq += len(txs)
        return out

    def revoke(self, rows):
        """Every row against the log as it stands before the call: 1 iff the ref is there and stores
        exactly the row's (txid, input_index, caller). The matched entries go; n_removed counts
        entries, so equal rows count once."""
        revoked = [1 if self.log.get(_key(ref)) == _by(by) else 0 for ref, by in rows]
        gone = {_key(ref) for (ref, _), r in zip(rows, revoked) if r}
        for r in gone:
            del self.log[r]
            del self.seq[r]
        return revoked, len(gone)

    def export(self, since_seq=0):
        """[(ref, by, seq)] of every entry with seq >= since_seq; the order means nothing."""
        return [(r, by, self.seq[r]) for r, by in self.log.items() if self.seq[r] >= since_seq]
