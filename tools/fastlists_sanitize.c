/* Stand-alone check of csrc/fastlists.c under AddressSanitizer + UBSan (`make -C csrc sanitize-fastlists`): this program embeds the
 * interpreter, has the helper compiled in (no extension is loaded, nothing is preloaded), and walks the two-phase construction the way
 * tests/test_fastlists_two_phase_cpu.py does -- fills in 1..3 ranges in both orders, tracked and untracked rows, every refusal, shells
 * dropped unfilled and half filled.  Run with PYTHONMALLOC=malloc so that every list body and int is a heap block the sanitizer sees
 * (the Makefile target sets it; leak detection is off because the interpreter itself does not free everything at exit).  CPU only. */
#define PY_SSIZE_T_CLEAN
#include <Python.h>
extern PyObject *PyInit__nlsh_fastlists(void);
static const char *script =
"import gc, array, _nlsh_fastlists as m\n"
"def block(vals, shape):\n"
"    return memoryview(array.array('i', vals)).cast('B').cast('i', shape=shape)\n"
"for Q, k in ((1, 1), (257, 10), (100, 64)):\n"
"    vals = [((i * 2654435761) % (2**31 + 1)) - 1 for i in range(Q * k)]\n"
"    cnts = [(i * 97) % 5000 for i in range(Q)]\n"
"    want = [vals[i * k:(i + 1) * k] for i in range(Q)]\n"
"    for parts in (1, 2, 3):\n"
"        for rev in (False, True):\n"
"            for untrack in (0, 1):\n"
"                outer, counts = m.rows_alloc(Q, k), [0] * Q\n"
"                bounds = [(Q * c // parts, Q * (c + 1) // parts) for c in range(parts)]\n"
"                for lo, hi in (b for b in (bounds[::-1] if rev else bounds) if b[1] > b[0]):\n"
"                    m.rows_fill(outer, lo, hi, block(vals[lo * k:hi * k], [hi - lo, k]), block(cnts[lo:hi], [hi - lo]), counts, untrack)\n"
"                assert outer == want and counts == cnts and gc.is_tracked(outer)\n"
"                gc.collect()\n"
"Q, k = 40, 6\n"
"vals, cnts = list(range(Q * k)), list(range(Q))\n"
"for _ in range(50):\n"
"    m.rows_alloc(Q, k)\n"
"    o, c = m.rows_alloc(Q, k), [0] * Q\n"
"    m.rows_fill(o, 10, 30, block(vals[60:180], [20, k]), block(cnts[10:30], [20]), c)\n"
"    for bad in (lambda: m.rows_fill(o, 0, 10, block(vals[:54], [9, k]), block(cnts[:10], [10]), c),\n"
"                lambda: m.rows_fill(o, 0, 10, block(vals[:60], [10, k]), block(cnts[:9], [9]), c),\n"
"                lambda: m.rows_fill(o, 5, 4, block(vals[:6], [1, k]), block(cnts[:1], [1]), c),\n"
"                lambda: m.rows_fill(o, 30, Q + 1, block(vals[:66], [11, k]), block(cnts[:11], [11]), c),\n"
"                lambda: m.rows_fill(o, 0, 10, block(vals[:70], [10, k + 1]), block(cnts[:10], [10]), c),\n"
"                lambda: m.rows_fill(o, 5, 15, block(vals[:60], [10, k]), block(cnts[:10], [10]), c),\n"
"                lambda: m.rows_fill(o, 0, 10, block(vals[:60], [10, k]), block(cnts[:10], [10]), [0] * 3)):\n"
"        try:\n"
"            bad()\n"
"        except ValueError:\n"
"            pass\n"
"        else:\n"
"            raise SystemExit('not refused')\n"
"    del o\n"
"    gc.collect()\n"
"print('embedded run ok')\n";
int main(void) {
    PyImport_AppendInittab("_nlsh_fastlists", PyInit__nlsh_fastlists);
    Py_Initialize();
    int rc = PyRun_SimpleString(script);
    if (Py_FinalizeEx() < 0) rc = 1;
    return rc ? 1 : 0;
}
