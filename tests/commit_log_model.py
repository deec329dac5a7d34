"""Plain-Python model of the notary's uniqueness check, one transaction at a time over a
dict -- the specification of the GPU commit log (K16, corda_amd/csrc/commit_log.hip).

It restates, for a non-validating notary's service flow (NotaryFlow.kt:98-104),

  TrustedAuthorityNotaryService.validateTimeWindow   NotaryService.kt:44-47
    TimeWindowChecker.isValid                        TimeWindowChecker.kt:14-25
  TrustedAuthorityNotaryService.commitInputStates    NotaryService.kt:53-67
    PersistentUniquenessProvider.commit              PersistentUniquenessProvider.kt:62-82

The reference holds no known-answer vectors for this (PersistentUniquenessProviderTests.kt:35-59
has two structural cases), so the checker is this restatement: the provider's map is a dict, its
lock is the order of the loop.

  commit(states, txId, callerIdentity):
      conflictingStates = {ref: committedStates[ref] for ref in states if ref in committedStates}
      if conflictingStates: throw UniquenessException(Conflict(conflictingStates))
      states.forEachIndexed { i, ref -> committedStates[ref] = ConsumingTx(txId, i, callerIdentity) }
  commitInputStates(inputs, txId, caller):
      try commit(...) catch UniquenessException e:
          conflicts = inputs.filterIndexed { i, ref ->
              e.error.stateHistory[ref] != null && e.error.stateHistory[ref] != ConsumingTx(txId, i, caller) }
          if conflicts.isNotEmpty(): throw NotaryException(Conflict(txId, signed stateHistory))
          # else: already committed by this very request -- return, the notary signs again

The comparison is per position i, and a ref listed twice is stored with its LAST position (the
puts run in list order): such a transaction commits and then conflicts with itself on
resubmission, its earlier position no longer equal to the stored index.
"""
OK, COMMIT_CONFLICT, COMMIT_TIME_WINDOW_INVALID, COMMIT_SKIPPED = 0, 16, 17, 18
REF_ABSENT, REF_SELF, REF_OTHER = 0, 1, 2


def window_valid(window, now_ns, tolerance_ns):
    """TimeWindowChecker.isValid (:22-23): window None or (from or None, until or None), exact ints."""
    if window is None:
        return True
    frm, until = window
    if until is not None and now_ns - until > tolerance_ns:
        return False
    if frm is not None and frm - now_ns > tolerance_ns:
        return False
    return True


class CommitLogModel:
    """committedStates: {(txhash, index): (txid, input_index, caller)}."""

    def __init__(self):
        self.log = {}

    def load(self, rows):
        """rows = [(ref, consuming_tx)]; returns how many refs were present already."""
        dup = 0
        for ref, by in rows:
            ref = (bytes(ref[0]), int(ref[1]))
            if ref in self.log:
                dup += 1
            else:
                self.log[ref] = (bytes(by[0]), int(by[1]), int(by[2]))
        return dup

    def commit_one(self, txid, caller, refs):
        """One commitInputStates call: (status, committed, ref_state, ref_by)."""
        refs = [(bytes(h), int(i)) for h, i in refs]
        present = [self.log.get(r) for r in refs]
        state = [REF_ABSENT if p is None else (REF_SELF if p == (txid, i, caller) else REF_OTHER)
                 for i, p in enumerate(present)]
        if all(p is None for p in present):
            for i, r in enumerate(refs):
                self.log[r] = (txid, i, caller)
            return OK, 1, [REF_ABSENT] * len(refs), [None] * len(refs)
        if all(s != REF_OTHER for s in state):
            return OK, 0, state, present
        return COMMIT_CONFLICT, 0, state, present

    def commit_batch(self, txs, now_ns=0, tolerance_ns=0, gate=None):
        """txs[t] = (txid, caller, refs, window), in batch order. Returns (tx_status, committed,
        ref_state, ref_by), the last two one list per transaction."""
        status, committed, states, bys = [], [], [], []
        for t, (txid, caller, refs, window) in enumerate(txs):
            if gate is not None and gate[t]:
                r = (COMMIT_SKIPPED, 0, [REF_ABSENT] * len(refs), [None] * len(refs))
            elif not window_valid(window, now_ns, tolerance_ns):
                r = (COMMIT_TIME_WINDOW_INVALID, 0, [REF_ABSENT] * len(refs), [None] * len(refs))
            else:
                r = self.commit_one(bytes(txid), int(caller), refs)
            status.append(r[0])
            committed.append(r[1])
            states.append(r[2])
            bys.append(r[3])
        return status, committed, states, bys
