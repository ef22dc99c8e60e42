"""The warp stream's rule (include/world_class_warp_stream.h) in Python integers and floats, written from the header's text alone:
the committed count by its predicate, the split of a push into unread and consumed rows and into outputs, and a stream as a list of
pushes over tests/warp_rule.py's map_position."""
import math

import warp_rule as W


def committed(entries, out_per_entry):
    """c(E): the n >= 0 with n / out_per_entry <= E - 1, c(0) = 0 -- the predicate, walked from the product's neighbourhood"""
    if entries < 1:
        return 0
    last = float(entries - 1)
    inside = lambda n: float(n) / out_per_entry <= last
    n = max(int(math.floor(last * out_per_entry)) - 2, 0)
    while not inside(n):   # (n = 0 is inside)
        n -= 1
    while inside(n + 1):
        n += 1
    return n + 1


def committed_by_brute_force(entries, out_per_entry):
    """the same without the product: every n from 0 until the predicate fails"""
    if entries < 1:
        return 0
    n = 0
    while float(n) / out_per_entry <= float(entries - 1):
        n += 1
    return n


def push_split(rows_before, n_rows, delay):
    """(unread, consumed): of a push's n_rows doubles the first `unread` are not read and the last `consumed` are map entries"""
    consumed = max(rows_before + n_rows - delay, 0) - max(rows_before - delay, 0)
    return n_rows - consumed, consumed


def flush_split(rows, delay):
    """(tail length, consumed): the tail holds min(D + 1, n) doubles, the last min(D, n) of them are the remaining entries"""
    return min(delay + 1, rows), min(delay, rows)


class Stream:
    """one stream since its reset: push(rows) and flush(tail) return the positions of the outputs they commit"""

    def __init__(self, delay, out_per_entry, in_per_unit):
        self.delay, self.ope, self.ipu = delay, out_per_entry, in_per_unit
        self.rows = 0
        self.entries = []   # every consumed entry (the model keeps them all; the handle carries the last one only)
        self.done = 0
        self.ended = False

    def _commit(self, new_entries):
        self.entries += [float(v) for v in new_entries]
        upto = committed(len(self.entries), self.ope)
        # by the prefix property the map of the entries so far gives these outputs what every longer map gives them
        pos = [W.map_position(self.entries, self.ope, self.ipu, n) for n in range(self.done, upto)]
        self.done = upto
        return pos

    def push(self, rows):
        assert not self.ended
        unread, consumed = push_split(self.rows, len(rows), self.delay)
        self.rows += len(rows)
        return self._commit(rows[unread:]) if consumed else []

    def flush(self, tail):
        assert not self.ended and self.delay > 0 and self.rows > 0
        length, consumed = flush_split(self.rows, self.delay)
        assert len(tail) == length
        self.ended = True
        return self._commit(tail[length - consumed:])


def settled_rows(entries, delay, filler=-777.0):
    """what an alignment stream with lag `delay` hands over for a voice whose rows have these positions: (the pushed doubles, the
    tail).  Row i >= delay holds entry i - delay, a row below holds a filler that nothing may read; the tail is the last
    min(delay + 1, n) entries"""
    n = len(entries)
    rows = [filler] * min(delay, n) + [float(v) for v in entries[:max(n - delay, 0)]]
    tail = [float(v) for v in entries[n - min(delay + 1, n):]] if delay > 0 and n > 0 else []
    return rows, tail
