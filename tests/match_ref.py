"""Sequential statement of `match` on columns -- test infrastructure, the role tests/extract_ref.py has
for template extraction.  Plain Python floats (float64), one pass per transmitter:

1. per txid, in input (= timestamp) order, a detection opens a new group when there is no group yet or
   when `timestamp[j] > timestamp[leader] + window`; otherwise it joins the open group;
2. inside a group the first detection of a receiver is its entry; a further one, j, records the
   collision (entry so far, j) and the entry becomes the earlier one only if its energy is strictly
   larger (a tie, or a NaN on either side: j);
3. groups are listed by their leader's input index; entries in the order their receivers first appeared
   (dict insertion order); fewer than `min_match` entries: the leader alone is a miss.
"""


def match_ref(rxid, txid, timestamp, energy, window, min_match=2):
    """-> (matches: list of lists, misses: list, collisions: list of (entry so far, j))."""
    rxid, txid = [int(v) for v in rxid], [int(v) for v in txid]
    timestamp, energy = [float(v) for v in timestamp], [float(v) for v in energy]
    window = float(window)
    members = {}
    for j, tx in enumerate(txid):
        members.setdefault(tx, []).append(j)
    groups = []          # (leader, {rxid: entry}, [collisions])
    for indices in members.values():
        leader = None
        for j in indices:
            if leader is None or timestamp[j] > timestamp[leader] + window:
                leader, entry, collided = j, {}, []
                groups.append((leader, entry, collided))
            before = entry.get(rxid[j])
            if before is not None:
                collided.append((before, j))
            entry[rxid[j]] = before if before is not None and energy[before] > energy[j] else j
    groups.sort(key=lambda g: g[0])
    matches = [list(entry.values()) for _, entry, _ in groups if len(entry) >= min_match]
    misses = [leader for leader, entry, _ in groups if len(entry) < min_match]
    collisions = [pair for _, _, collided in groups for pair in collided]
    return matches, misses, collisions


def to_csr(matches):
    """list of lists -> (ptr, idx) as plain lists."""
    ptr, idx = [0], []
    for m in matches:
        idx.extend(m)
        ptr.append(len(idx))
    return ptr, idx


def from_csr(ptr, idx):
    ptr, idx = [int(v) for v in ptr], [int(v) for v in idx]
    return [idx[a:b] for a, b in zip(ptr[:-1], ptr[1:])]
