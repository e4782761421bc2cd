"""Multi-table index: T independently trained hashes over ONE corpus, each probed lightly, their candidates united.

A `MultiTableIndexer` owns T ordinary `Indexer`s (`compat=False`, `algo="tiled"`) over the same rows and the same global row ids.  A
query asks every table for its top-k with the 64-bit sort keys `monotone(dist) << 32 | id` and merges the T lists with ONE
`nlsh_merge_topk_unique` call, which counts equal keys once.  The result is EXACTLY the top-k by (distance bits, id) of a scan over the
union of the T candidate sets, not an approximation of it: within one table a query's candidates are distinct rows, so every member of
the union's k best is among the k best of at least one table, and the same row reached through two tables carries the same key because
the tiled schedule's distance of a (query, row) pair is a function of the two vectors alone -- which is why the tiled schedule is
forced at every batch size, a one-query batch included.

Cost, stated plainly:
  - memory is T bucket-sorted copies of the corpus: `storage="uint8"` / `"float16"` make them affordable (four uint8 tables cost what
    one float32 index costs);
  - a row that sits in the probed buckets of several tables is scored once per table that finds it; `ncand` is that sum (scored
    pairs, with multiplicity), not the size of the union;
  - the tables run back to back on the current stream, then the merge; nothing runs on parallel streams;
  - `hash_times`, `probes` and `candidate_budget` are PER TABLE.

There is no pipelined, graph-slot or sharded multi-table entry point: `QueryPipeline`, the step slots and the distributed builds take
an `Indexer`, and a `MultiTableIndexer` is not one.  Run those per table if needed, or use this class's eager calls.
"""
import weakref
from typing import List, Optional, Sequence, Tuple

import torch

from . import _capi
from .data import metric_of
from .indexer import Indexer, RowFilter, _STORAGES, _stream
from .refine import RefineStore, checked_refine, stage_one_k


class MultiRowFilter:
    """A row filter of ONE `MultiTableIndexer` in ONE generation (`MultiTableIndexer.row_filter` builds it): `filters`, one `RowFilter`
    per table -- the bitset is in each table's own sorted-row order, so the tables cannot share one -- `n_allowed`, how many rows it
    allows, and `generation`, the multi-table index's when it was built.  Stale after an effective `add` / `remove` / `update`."""

    __slots__ = ("filters", "n_allowed", "generation", "_index")

    def __init__(self, index, filters, generation):
        self.filters = tuple(filters)
        self.n_allowed = self.filters[0].n_allowed
        self.generation = int(generation)
        self._index = weakref.ref(index)

    def __repr__(self):
        return f"MultiRowFilter(tables={len(self.filters)}, n_allowed={self.n_allowed}, generation={self.generation})"


class MultiTableIndexer:
    """T hash tables over one corpus, queried as one index (module docstring).

    hashings: a sequence of 1 .. 16 (`_capi.MAX_TABLES`) hashers, all different objects (the same hasher twice is the same table
    twice: twice the work for no candidate more).  corpus_keys: None, or one int32 key tensor per table (`Indexer`'s `corpus_keys=`).
    Every other argument is `Indexer`'s and goes to every table; `compat=False` and `algo="tiled"` are fixed.  `row_ids` / `id_base`
    name the rows as in `Indexer` (a rebuilt index keeps its ids through them).  Metric 'l2' or 'cosine' only.
    `.tables` is the list of tables.  Results, candidate counts and limits: `query_tensors`."""

    refine, refine_factor, refine_store = None, 4, None     # no second stage unless the constructor is given refine=

    def __init__(self, hashings, candidate_vectors_gpu, distance_func, metric: Optional[str] = None, storage: Optional[str] = None,
                 l2_form: str = "exact", row_align: int = 4, window_rows: Optional[int] = None, corpus_keys=None,
                 row_ids: Optional[torch.Tensor] = None, id_base: int = 0, quantiser=None, refine: Optional[str] = None,
                 refine_factor: int = 4, tags: Optional[torch.Tensor] = None, pq_dsub: Optional[int] = None, pq_dim: Optional[int] = None):
        # tags: None | int64 [N] = `Indexer`'s `tags=`, handed to every table (each keeps them in its own sorted order: 8 bytes per row
        # and table); the queries then take `tag_mask=` / `tag_match=`
        # refine: None | "device" | "host" = ONE store of the caller's float32 rows behind the de-duplicating merge:
        # every table runs at k1, the merge keeps k1 distinct candidates and one re-rank cuts to k.  The tables themselves hold no store.
        self.refine, self.refine_factor = checked_refine(refine, refine_factor)
        self.refine_store = None
        if self.refine is not None and row_ids is not None:
            raise ValueError("refine= needs the default row ids (id_base + row): the refine store addresses a row by id - id_base, "
                             "row_ids= names rows freely")
        if quantiser is not None and storage not in ("sq8", "pq"):
            raise ValueError(f"quantiser= belongs to storage='sq8' (lo, step) or storage='pq' (a codebook), not storage={storage!r}")
        if (pq_dsub is not None or pq_dim is not None) and storage != "pq":
            raise ValueError(f"pq_dsub= / pq_dim= belong to storage='pq', not storage={storage!r}")
        hashings = list(hashings)
        if not hashings:
            raise ValueError("hashings is empty: a multi-table index needs at least one hasher")
        if len(hashings) > _capi.MAX_TABLES:
            raise ValueError(f"{len(hashings)} hashers: a multi-table index takes at most {_capi.MAX_TABLES} (NLSH_MAX_TABLES)")
        for i, h in enumerate(hashings):
            for j in range(i):
                if hashings[j] is h:
                    raise ValueError(f"hashings[{j}] and hashings[{i}] are the same object: two tables of one hasher hold the same "
                                     "buckets (train one hasher per table)")
        if corpus_keys is not None:
            corpus_keys = list(corpus_keys)
            if len(corpus_keys) != len(hashings):
                raise ValueError(f"corpus_keys must hold one key tensor per table: {len(corpus_keys)} given for {len(hashings)} hashers")
        if storage is not None and storage not in _STORAGES:
            raise ValueError(f"storage must be None or one of {tuple(_STORAGES)}, got {storage!r}")
        self.metric = metric or metric_of(distance_func)
        if self.metric not in ("l2", "cosine"):
            raise NotImplementedError("a multi-table index needs metric 'l2' or 'cosine': its merge rests on the tiled schedule's distance bits")
        # storage="sq8": ONE quantiser for all tables -- the given one, or the one the first table trains on the corpus -- so that every
        # table holds the same decoded rows and a row's distance has one value whichever table finds it (the merge rests on that).
        # storage="pq": ONE codebook for all tables in the same way, trained (by the first table) or given once.
        self.tables: List[Indexer] = []
        for t, h in enumerate(hashings):
            kw = {} if storage != "sq8" else {"quantiser": quantiser if t == 0 else self.tables[0].quantiser}
            if storage == "pq":
                kw = {"quantiser": quantiser if t == 0 else self.tables[0].codebook, "pq_dsub": pq_dsub, "pq_dim": pq_dim}
            self.tables.append(Indexer(h, candidate_vectors_gpu, distance_func, compat=False, metric=self.metric, algo="tiled", storage=storage,
                                       l2_form=l2_form, row_align=row_align, window_rows=window_rows, row_ids=row_ids, id_base=id_base,
                                       corpus_keys=None if corpus_keys is None else corpus_keys[t], tags=tags, **kw))
        self.storage = self.tables[0].storage
        if self.refine is not None:
            originals = candidate_vectors_gpu
            if self.storage in ("sq8", "pq") and originals.dtype == torch.uint8:
                originals = self.tables[0]._dequantised(originals)
            self.refine_store = RefineStore(originals, self.metric, id_base=id_base, where=self.refine, row_align=row_align)
        self.generation = 0         # +1 per effective add / remove / update: a MultiRowFilter of an older one is stale

    # ------------------------------------------------------------------ shape
    @property
    def n_tables(self):
        return len(self.tables)

    @property
    def n_rows(self):
        return int(self.tables[0].gid.shape[0])

    @property
    def next_id(self):
        """The id `add` gives its first row when the caller names none (one counter for all tables: they move together)."""
        return max(t.next_id for t in self.tables)

    # ------------------------------------------------------------------ queries
    def _checked_filter(self, filter):
        """`filter=` of a call, checked before anything is launched -> one RowFilter (or None) per table."""
        if filter is None:
            return [None] * len(self.tables)
        if isinstance(filter, RowFilter):
            raise ValueError("filter is a RowFilter of a single table: its bitset is in that table's row order and the other tables cannot "
                             "read it; build a MultiRowFilter with this index's row_filter()")
        if not isinstance(filter, MultiRowFilter):
            raise ValueError(f"filter must be None or a MultiRowFilter built by this index's row_filter(), got {type(filter).__name__}")
        if filter._index() is not self:
            raise ValueError("filter was built by another index: a MultiRowFilter addresses the sorted rows of the tables that built it")
        if filter.generation != self.generation:
            raise ValueError(f"stale filter: built at generation {filter.generation}, the index is at {self.generation} "
                             "(add / remove / update move rows); build a new one with row_filter()")
        return list(filter.filters)

    @staticmethod
    def _checked_k(k):
        if not 1 <= int(k) <= _capi.MAX_K_TILED:
            raise ValueError(f"k={k}: a multi-table query takes k in [1, {_capi.MAX_K_TILED}] (NLSH_MAX_K_TILED, the tiled schedule's limit)")
        return int(k)

    def query_tensors(self, query_vectors, k=10, hash_times=10, seed=None, probes=None, candidate_budget=None, filter=None,
                      want_keys=False, refine_k=None, tag_mask=None, tag_match="any"):
        """Device-resident query -> (dist [Q, k] float32, idx [Q, k] int32, ncand [Q] int32[, keys64 [Q, k] int64]).
        Every table answers `Indexer.query_tensors(..., want_keys=True)` with these arguments, one after the other on the current
        stream -- `hash_times`, `probes`, `candidate_budget` and `seed` are therefore PER TABLE -- and one `nlsh_merge_topk_unique` call
        merges the T lists: the k best DISTINCT (distance bits, id) keys, -1 / +inf / ~0 behind a query with fewer than k distinct
        candidates.  `ncand` is the sum of the tables' counts: scored (query, row) pairs, a row found by two tables counted twice.
        filter: a `MultiRowFilter` of this index (`row_filter()`); table t is handed its own bitset.  k <= 256.
        tag_mask / tag_match (an index built with `tags=` only): `Indexer.query_tensors`' per-query tag filters, handed to every table.
        refine_k (an index built with `refine=` only; None = min(256, max(k, refine_factor * k)), 0 = off for this call): every table runs
        at k1, the merge keeps the k1 best distinct candidates and ONE `nlsh_rerank_topk` launch returns the k best of them by their exact
        float32 distance to the original rows; `ncand` stays the merge's sum, keys64 are the re-rank's."""
        k = self._checked_k(k)
        filters = self._checked_filter(filter)
        if self.refine_store is None and refine_k:
            raise ValueError("refine_k= needs an index built with refine='device' or 'host'")
        k1 = stage_one_k(k, self.refine_factor, refine_k) if self.refine_store is not None else 0
        if k1:
            _, idx1, nc = self.query_tensors(query_vectors, k=k1, hash_times=hash_times, seed=seed, probes=probes,
                                             candidate_budget=candidate_budget, filter=filter, refine_k=0, tag_mask=tag_mask,
                                             tag_match=tag_match)
            dist, idx, _, keys64 = self.refine_store.rerank(self.tables[0]._as_queries(query_vectors), idx1, k, want_keys=True)
            return (dist, idx, nc, keys64) if want_keys else (dist, idx, nc)
        q = self.tables[0]._as_queries(query_vectors)     # made contiguous float32 once, not once per table
        keys, counts = [], []
        for table, f in zip(self.tables, filters):
            _, _, nc, k64 = table.query_tensors(q, k=k, hash_times=hash_times, seed=seed, want_keys=True, probes=probes,
                                                candidate_budget=candidate_budget, filter=f, tag_mask=tag_mask, tag_match=tag_match)
            keys.append(k64)
            counts.append(nc)
        return self._merge(torch.stack(keys), torch.stack(counts), k, want_keys)

    @staticmethod
    def _merge(keys_all, counts_all, k, want_keys):
        """keys_all int64 [T, Q, k] (the tables' sort keys), counts_all int32 [T, Q] -> the merged (dist, idx, ncand[, keys64])."""
        T, Q, _ = keys_all.shape
        dev = keys_all.device
        out_dist = torch.empty((Q, k), dtype=torch.float32, device=dev)
        out_idx = torch.empty((Q, k), dtype=torch.int32, device=dev)
        out_nc = torch.empty((Q,), dtype=torch.int32, device=dev)
        out_keys = torch.empty((Q, k), dtype=torch.int64, device=dev) if want_keys else None
        _capi.check(_capi.lib().nlsh_merge_topk_unique(_capi.ptr(keys_all), k, T, Q, k, _capi.ptr(counts_all), _capi.ptr(out_dist),
                                                       _capi.ptr(out_idx), _capi.ptr(out_keys), _capi.ptr(out_nc), _stream(dev)))
        return (out_dist, out_idx, out_nc, out_keys) if want_keys else (out_dist, out_idx, out_nc)

    def query(self, query_vectors, k=10, hash_times=10, seed=None, probes=None, candidate_budget=None,
              filter=None, tag_mask=None, tag_match="any") -> Tuple[List[List[int]], List[int]]:
        """`Indexer.query` with `compat=False`: (id lists in (distance, id) order, candidate counts).  A list holds min(k, distinct
        candidates) ids -- its length comes from the sort keys, -1 being a legal row id -- so a query with fewer than k distinct
        candidates gets a short list and one with none an empty list: the reference's "fewer than k candidates -> rows of the last key"
        rule (F7) describes one hash table and is not applied here, as on filtered calls.  The counts are `query_tensors`' sums."""
        _, idx, ncand, keys64 = self.query_tensors(query_vectors, k=k, hash_times=hash_times, seed=seed, probes=probes,
                                                   candidate_budget=candidate_budget, filter=filter, want_keys=True, tag_mask=tag_mask,
                                                   tag_match=tag_match)
        return self.tables[0]._filtered_lists(idx, ncand, keys64)

    # ------------------------------------------------------------------ mutation
    def add(self, vectors, ids=None, tags=None) -> torch.Tensor:
        """Add rows [M, d] to EVERY table -> their int32 ids (device).  The ids are fixed once -- `ids`, or `next_id ..` -- and handed
        to each table explicitly, so a row has one id everywhere; each table hashes the rows with its own hasher."""
        return self.update(add=vectors, add_ids=ids, add_tags=tags)[0]

    def remove(self, ids) -> int:
        """Remove the rows with these ids from every table -> how many rows went."""
        return self.update(remove=ids)[1]

    def update(self, add=None, add_ids=None, remove=None, add_tags=None) -> Tuple[torch.Tensor, int]:
        """`Indexer.update` on every table: `remove` and `add` in one pass per table -> (ids of the added rows, rows removed).  After
        the call every table holds the same id set.  A `MultiRowFilter` built before an effective call is stale."""
        first = self.tables[0]
        if self.refine_store is not None and add_ids is not None:
            raise ValueError("add(ids=...) on an index with refine=: the refine store addresses a row by id - id_base, so added rows take "
                             "the default ids (nothing was changed)")
        if add is not None:
            for t, table in enumerate(self.tables):     # what a LATER table would refuse is refused before the first one changes
                needs_train = getattr(table._hashing, "_needs_train_forward", None)
                if needs_train is not None and needs_train():
                    raise _capi.NlshHipError(_capi.E_UNSUPPORTED, f"add() needs eval mode for BatchNorm encoders (train_mode(False)): "
                                                                  f"hashings[{t}] is in train mode")
            if add_ids is None and isinstance(add, torch.Tensor) and add.dim() == 2 and add.shape[0] and first.row_ids is None:
                M, start = int(add.shape[0]), self.next_id
                if start + M - 1 > 0x7FFFFFFF:
                    raise ValueError("row ids are int32: next_id + M exceeds 2^31 - 1")
                add_ids = torch.arange(start, start + M, dtype=torch.int32, device=first.gid.device)
        before = [table.generation for table in self.tables]
        result = None
        for t, table in enumerate(self.tables):
            try:
                got = table.update(add=add, add_ids=add_ids, remove=remove, add_tags=add_tags)
            except Exception as exc:
                if t:       # the arguments are the same for every table, so a refusal comes from the first one, nothing changed
                    raise RuntimeError(f"table {t} refused an update that tables 0..{t - 1} applied; the tables no longer hold the "
                                       "same rows: rebuild the MultiTableIndexer") from exc
                raise
            result = got if result is None else result
        if any(table.generation != g for table, g in zip(self.tables, before)):
            self.generation += 1
        if self.refine_store is not None and result is not None and int(result[0].shape[0]):
            originals = add
            if self.storage in ("sq8", "pq") and add.dtype == torch.uint8:
                originals = first._dequantised(add)
            assert int(result[0][0].item()) == self.refine_store.id_base + self.refine_store.n_rows
            self.refine_store.append(originals)      # once: the tables share the store
        return result

    def set_tags(self, ids, tags) -> int:
        """`Indexer.set_tags` on every table -> how many rows were found (the tables hold the same ids)."""
        return [table.set_tags(ids, tags) for table in self.tables][0]

    # ------------------------------------------------------------------ filters
    def row_filter(self, allow=None, deny=None, mask=None) -> MultiRowFilter:
        """`Indexer.row_filter` on every table (exactly one of `allow=`, `deny=`, `mask=`) -> a `MultiRowFilter` for `filter=` of
        `query_tensors` / `query`.  T bitsets: each is in its table's own sorted-row order."""
        return MultiRowFilter(self, [table.row_filter(allow=allow, deny=deny, mask=mask) for table in self.tables], self.generation)
