"""What a scene must do to a table for its compaction (csrc/table_compact.h: 256 rows per workgroup, a scan over the workgroups' counts)
to be exercised across workgroups, computed from the ids of a table before and after rows left it.  The CPU tests assert these on the
restatements' tables; the GPU tests then compare the device's tables with the same restatements bit for bit."""
import numpy as np

BLOCK = 256


def removed_rows(before_ids, after_ids):
    """rows of the table before, in ascending order, whose id the table after no longer holds"""
    return np.flatnonzero(~np.isin(np.asarray(before_ids), np.asarray(after_ids)))


def crosses_blocks(before_ids, after_ids):
    """-> (the removed rows lie in at least two 256-row blocks, a kept row in a later block follows a removed one): the first makes two
    workgroups' counts differ from 256, the second makes a later workgroup's offset depend on an earlier one's count"""
    gone = removed_rows(before_ids, after_ids)
    if len(gone) == 0:
        return False, False
    kept = np.setdiff1d(np.arange(len(before_ids)), gone)
    return len(np.unique(gone // BLOCK)) >= 2, bool(len(kept)) and int(kept[-1]) // BLOCK > int(gone[0]) // BLOCK
