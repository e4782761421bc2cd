/* Host-side helper of the Python facade (nlsh_amd/indexer.py): the reference's Indexer.query returns List[List[int]]
 * (nlsh/indexer.py:90-96: `indexes.tolist()` per query), i.e. 10^5 Python ints in 10^4 lists per 10^4-query batch, and building
 * them is the longest stage of a query() call once the device side takes 0.37 ms.  numpy's `ndarray.tolist()` goes through its
 * generic per-element getitem; this is the same construction as one tight loop (PyList_New + PyLong_FromLong), ~20 % faster.
 * Plain CPython C API, no GPU code; optional: the facade falls back to `ndarray.tolist()` when the module is not built.
 * Same result, element for element (tests/test_host_cpu.py).
 *
 * OPT-IN (fourth argument, default 0; `Indexer.untracked_results`): the inner lists are handed out UNTRACKED by the cyclic garbage
 * collector (PyObject_GC_UnTrack).  A list of ints cannot be part of a reference cycle, and CPython itself untracks tuples and dicts of
 * atomic objects for the same reason; 10^4 tracked young lists per call are what makes the collector's next generation-0 pass cost
 * 0.26 ms, and untracked they are invisible to it.  But CPython never untracks LISTS: a caller that later builds a
 * reference cycle through such a row (row.append(obj_that_references_row)) would leak it, so by default the rows are ordinary tracked
 * lists, exactly what `.tolist()` returns in the reference (nlsh/indexer.py:91); r03 had this on whenever the helper was built. */
#define PY_SSIZE_T_CLEAN
#include <Python.h>
#include <stdint.h>

/* rows_to_lists(buffer of int32 [Q, k] C-contiguous, Q, k, untrack=0) -> [[int] * k] * Q */
static PyObject *rows_to_lists(PyObject *self, PyObject *args) {
    Py_buffer view;
    Py_ssize_t Q, k;
    int untrack = 0;
    (void)self;
    if (!PyArg_ParseTuple(args, "y*nn|p", &view, &Q, &k, &untrack)) return NULL;
    if (Q < 0 || k < 0 || view.len < Q * k * 4) {
        PyBuffer_Release(&view);
        PyErr_SetString(PyExc_ValueError, "rows_to_lists: buffer smaller than Q * k int32");
        return NULL;
    }
    const int32_t *p = (const int32_t *)view.buf;
    PyObject *outer = PyList_New(Q);
    if (!outer) { PyBuffer_Release(&view); return NULL; }
    for (Py_ssize_t q = 0; q < Q; ++q) {
        PyObject *row = PyList_New(k);
        if (!row) { Py_DECREF(outer); PyBuffer_Release(&view); return NULL; }
        PyList_SET_ITEM(outer, q, row);   /* owned by outer from here: a failure below releases everything through it */
        for (Py_ssize_t j = 0; j < k; ++j) {
            PyObject *v = PyLong_FromLong((long)p[q * k + j]);
            if (!v) { Py_DECREF(outer); PyBuffer_Release(&view); return NULL; }
            PyList_SET_ITEM(row, j, v);
        }
        if (untrack) PyObject_GC_UnTrack(row);
    }
    PyBuffer_Release(&view);
    return outer;
}

/* TWO-PHASE construction (Indexer._query): the containers of a batch's result do not depend on the ids, so the facade builds them
 * while the device still scans the first row range (`rows_alloc`) and stores each range's ids when its event completes (`rows_fill`).
 *
 * A SHELL is the outer list of Q inner lists of length k whose slots are still empty (NULL, as PyList_New leaves them).  Such a list
 * is not a valid Python object yet, so nothing may find it: every inner list is taken off the collector right after PyList_New, and
 * so is the outer list, for as long as one of its rows is unfilled.  The only reference to a shell is the one `rows_alloc` returns,
 * which the facade keeps in the frame of the running call; `gc.get_objects()`, `gc.get_referrers()` and a collection running in
 * another thread (the facade sleeps without the GIL between the phases) deal with tracked containers only and skip the shell and
 * its rows.  What is left is code that digs the shell out of that frame on purpose.  A filled row is an ordinary list and goes back
 * on the collector (unless `untrack`, the opt-in above); the outer list follows with the fill that leaves no row empty.
 * A shell that is dropped unfilled or half filled is released like any list: list deallocation skips empty slots.
 * Ints are created with their value (PyLong_FromLong) at fill time; no object is created early and patched. */

/* whether `row` is a list of this module's whose slots are still empty (slot 0 is written with the rest of the row, under the GIL) */
static int row_is_empty_shell(PyObject *row) {
    return PyList_CheckExact(row) && PyList_GET_SIZE(row) > 0 && PyList_GET_ITEM(row, 0) == NULL;
}

/* rows_alloc(Q, k) -> shell: [[<empty> * k] * Q], off the collector until filled.  k == 0 (or Q == 0): nothing is left to fill,
 * the lists are complete and ordinary (tracked) from the start. */
static PyObject *rows_alloc(PyObject *self, PyObject *args) {
    Py_ssize_t Q, k;
    (void)self;
    if (!PyArg_ParseTuple(args, "nn", &Q, &k)) return NULL;
    if (Q < 0 || k < 0) {
        PyErr_SetString(PyExc_ValueError, "rows_alloc: negative Q or k");
        return NULL;
    }
    PyObject *outer = PyList_New(Q);
    if (!outer) return NULL;
    if (Q > 0 && k > 0) PyObject_GC_UnTrack(outer);
    for (Py_ssize_t q = 0; q < Q; ++q) {
        PyObject *row = PyList_New(k);
        if (!row) { Py_DECREF(outer); return NULL; }
        if (k > 0) PyObject_GC_UnTrack(row);
        PyList_SET_ITEM(outer, q, row);
    }
    return outer;
}

/* a C-contiguous block of native int32 with the given shape (cols < 0: one dimension)?  The exporter states its own shape and item
 * type (numpy: 'i', or 'l' where long is 4 bytes), so a block of another row length or dtype is refused, not reinterpreted. */
static int is_int32_block(const Py_buffer *v, Py_ssize_t rows, Py_ssize_t cols) {
    const char *f = v->format ? v->format : "B";
    if (*f == '@' || *f == '=' || *f == (*(const char *)&(int){1} ? '<' : '>')) ++f;
    if (v->itemsize != 4 || !(f[0] == 'i' || f[0] == 'l') || f[1] != '\0') return 0;
    if (cols < 0) return v->ndim == 1 && v->shape[0] == rows;
    return v->ndim == 2 && v->shape[0] == rows && v->shape[1] == cols;
}

/* rows_fill(shell, lo, hi, ids: int32 [hi-lo, k] C-contiguous, counts: int32 [hi-lo], counts_out: list of len(shell), untrack=0) -> None
 * Rows [lo, hi) of the shell take their ids, counts_out[lo:hi] the counts as ints.  Everything is checked before anything is stored
 * (ValueError): the range, both blocks' shapes and item type, and every row of the range -- an exact list of the ids' row length
 * that is still empty.  If an id cannot be allocated the row it was meant for is emptied again, the rows before it stay filled, and
 * MemoryError is raised: the shell stays releasable (and refillable from that row on). */
static PyObject *rows_fill(PyObject *self, PyObject *args) {
    PyObject *outer, *counts_out, *ids_obj, *counts_obj, *result = NULL;
    Py_ssize_t lo, hi;
    Py_buffer ids, counts;
    int untrack = 0;
    (void)self;
    if (!PyArg_ParseTuple(args, "O!nnOOO!|p", &PyList_Type, &outer, &lo, &hi, &ids_obj, &counts_obj, &PyList_Type, &counts_out, &untrack)) return NULL;
    if (PyObject_GetBuffer(ids_obj, &ids, PyBUF_C_CONTIGUOUS | PyBUF_FORMAT) < 0) return NULL;
    if (PyObject_GetBuffer(counts_obj, &counts, PyBUF_C_CONTIGUOUS | PyBUF_FORMAT) < 0) { PyBuffer_Release(&ids); return NULL; }
    const Py_ssize_t Q = PyList_GET_SIZE(outer), k = ids.ndim == 2 ? ids.shape[1] : -1;
    const char *why = NULL;
    if (lo < 0 || lo > hi || hi > Q) why = "rows_fill: need 0 <= lo <= hi <= len(shell)";
    else if (PyList_GET_SIZE(counts_out) != Q) why = "rows_fill: counts_out is not a list of len(shell)";
    else if (k < 0 || !is_int32_block(&ids, hi - lo, k)) why = "rows_fill: ids are not a C-contiguous int32 block [hi - lo, k]";
    else if (!is_int32_block(&counts, hi - lo, -1)) why = "rows_fill: counts are not a C-contiguous int32 block [hi - lo]";
    for (Py_ssize_t q = lo; q < hi && !why; ++q) {
        PyObject *row = PyList_GET_ITEM(outer, q);
        if (!PyList_CheckExact(row) || PyList_GET_SIZE(row) != k) why = "rows_fill: a row of the range is not a list of the ids' row length";
        else if (k > 0 && !row_is_empty_shell(row)) why = "rows_fill: a row of the range is already filled";
    }
    if (why) {
        PyErr_SetString(PyExc_ValueError, why);
        goto done;
    }
    const int32_t *p = (const int32_t *)ids.buf, *c = (const int32_t *)counts.buf;
    for (Py_ssize_t q = lo; q < hi; ++q, p += k) {
        PyObject *row = PyList_GET_ITEM(outer, q);
        if (k > 0 && !row_is_empty_shell(row)) {   /* the same list twice in one range: only a caller that took a shell apart builds that */
            PyErr_SetString(PyExc_ValueError, "rows_fill: a row of the range is already filled");
            goto done;
        }
        for (Py_ssize_t j = 0; j < k; ++j) {
            PyObject *v = PyLong_FromLong((long)p[j]);
            if (!v) {               /* back to an empty row: a row is whole or empty, never in between, when this call returns */
                while (--j >= 0) {
                    PyObject *old = PyList_GET_ITEM(row, j);
                    PyList_SET_ITEM(row, j, NULL);
                    Py_DECREF(old);
                }
                goto done;
            }
            PyList_SET_ITEM(row, j, v);
        }
        if (untrack) {
            if (PyObject_GC_IsTracked(row)) PyObject_GC_UnTrack(row);
        } else if (!PyObject_GC_IsTracked(row)) {
            PyObject_GC_Track(row);
        }
    }
    /* the counts in a pass of their own, as `tolist()` makes them: a count created between two rows' ids sits among them in the
     * allocator's pools and outlives them, and releasing such a result measured slower than releasing a one-shot one */
    for (Py_ssize_t q = lo; q < hi; ++q) {
        PyObject *n = PyLong_FromLong((long)c[q - lo]);
        if (!n) goto done;      /* the rows are whole; the counts from here on keep what they held */
        PyObject *old = PyList_GET_ITEM(counts_out, q);
        PyList_SET_ITEM(counts_out, q, n);
        Py_XDECREF(old);
    }
    if (!PyObject_GC_IsTracked(outer)) {   /* the fill that leaves no row empty puts the outer list on the collector */
        Py_ssize_t q = lo == 0 ? hi : 0;    /* rows [lo, hi) were filled just now */
        while (q < Q && !row_is_empty_shell(PyList_GET_ITEM(outer, q))) q = (q + 1 == lo) ? hi : q + 1;
        if (q >= Q) PyObject_GC_Track(outer);
    }
    result = Py_None;
    Py_INCREF(result);
done:
    PyBuffer_Release(&ids);
    PyBuffer_Release(&counts);
    return result;
}

static PyMethodDef methods[] = {{"rows_to_lists", rows_to_lists, METH_VARARGS, "int32 [Q, k] buffer -> list of Q lists of k ints"},
                                {"rows_alloc", rows_alloc, METH_VARARGS, "(Q, k) -> shell: Q empty lists of length k, off the collector until filled"},
                                {"rows_fill", rows_fill, METH_VARARGS,
                                 "(shell, lo, hi, int32 [hi-lo, k] buffer, int32 [hi-lo] buffer, counts_out, untrack=0): fill rows [lo, hi)"},
                                {NULL, NULL, 0, NULL}};
static struct PyModuleDef module = {PyModuleDef_HEAD_INIT, "_nlsh_fastlists", NULL, -1, methods, NULL, NULL, NULL, NULL};
PyMODINIT_FUNC PyInit__nlsh_fastlists(void) { return PyModule_Create(&module); }
