// mexhost.cpp -- a test host for the MEX shims: a real implementation of exactly the prototypes in
// integration/mex_stub/mex.h (documented MEX / matrix C API semantics, nothing more), plus a flat C driver
// interface (mh_*) that tests/mexhost.py reaches through ctypes.  Test infrastructure only: nothing here ships.
//
// One shim + this file = one shared object (each shim defines mexFunction and its own static context).
//
// What the host does around a call, as MATLAB does: arrays created during the call and not returned in
// plhs[0 .. max(nlhs,1)-1] are freed afterwards, also after an error; mexErrMsgIdAndTxt leaves the call by a C++
// exception that mh_call catches.  What it checks, each reported as a host error (mh_error_*) and never a crash:
// mxDestroyArray twice on one array or on an input, a destroyed array or an input returned, a plhs slot beyond
// max(nlhs,1) written, an input whose bytes changed during the call (FNV-1a before / after), a typed accessor on
// the wrong class (an error under -R2018a), and a broken guard: every data buffer lies between two kGuard-byte
// zones filled with kFill, so a wrong size or leading dimension handed to the library shows as a changed guard.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <set>
#include <string>
#include <vector>

#include "mex.h"

namespace {

constexpr size_t kGuard = 64;
constexpr unsigned char kFill = 0xA5;
constexpr int kSlack = 16;  // plhs slots past max(nlhs,1) that a shim may (wrongly) write without corrupting the host

struct MexError {
    std::string id, msg;
};
struct HostAbort {};  // the call cannot go on (e.g. a typed accessor on the wrong class): already recorded

}  // namespace

struct mxArray_tag {
    mxClassID cls = mxUNKNOWN_CLASS;
    bool is_struct = false;
    size_t m = 0, n = 0, bytes = 0;
    unsigned char* raw = nullptr;  // kGuard | bytes | kGuard
    std::vector<std::string> fnames;
    std::vector<mxArray*> fvals;
    bool input = false;   // a prhs array (or a field of one) of the running call
    bool owned = false;   // a field of a struct: lives and dies with it
    unsigned char* data() const { return raw + kGuard; }
};

namespace {

std::set<mxArray*> g_live, g_dead;      // g_dead: headers of destroyed arrays, kept so that a second destroy is seen
std::vector<mxArray*> g_created;        // created during the running call
std::vector<mxArray*> g_out;            // the results of the last call
std::vector<std::string> g_errors;      // host errors
bool g_in_call = false;
int g_lock = 0, g_status = 0;
void (*g_exit_fcn)(void) = nullptr;     // one active exit function per MEX file (the documented rule)
std::string g_err_id, g_err_msg;

void host_error(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_errors.push_back(buf);
}

size_t elem_size(mxClassID c) {
    switch (c) {
        case mxLOGICAL_CLASS: return 1;
        case mxCHAR_CLASS: return 2;
        case mxDOUBLE_CLASS: return 8;
        case mxSINGLE_CLASS: return 4;
        case mxINT16_CLASS: return 2;
        case mxINT32_CLASS: return 4;
        default: return 0;
    }
}

mxArray* make(mxClassID cls, size_t m, size_t n) {
    const size_t es = elem_size(cls);
    if (!es) {
        host_error("array of unsupported class %d requested", (int)cls);
        throw HostAbort();
    }
    mxArray* a = new mxArray_tag();
    a->cls = cls;
    a->m = m;
    a->n = n;
    a->bytes = es * m * n;
    a->raw = (unsigned char*)std::malloc(a->bytes + 2 * kGuard);
    if (!a->raw) std::abort();
    std::memset(a->raw, kFill, kGuard);
    std::memset(a->raw + kGuard, 0, a->bytes);  // mxCreate*: zero-filled
    std::memset(a->raw + kGuard + a->bytes, kFill, kGuard);
    g_live.insert(a);
    if (g_in_call) g_created.push_back(a);
    return a;
}

mxArray* make_struct() {
    mxArray* a = new mxArray_tag();
    a->is_struct = true;
    a->m = a->n = 1;
    g_live.insert(a);
    if (g_in_call) g_created.push_back(a);
    return a;
}

bool guards_ok(const mxArray* a) {
    if (!a->raw) return true;
    for (size_t i = 0; i < kGuard; ++i)
        if (a->raw[i] != kFill || a->raw[kGuard + a->bytes + i] != kFill) return false;
    return true;
}

void check_guards(const mxArray* a, const char* when) {
    if (!guards_ok(a)) host_error("guard zone of a %zu x %zu array (class %d) overwritten (%s)", a->m, a->n, (int)a->cls, when);
    for (const mxArray* f : a->fvals)
        if (f) check_guards(f, when);
}

// frees the storage; the header goes to g_dead when `tomb` (a destroy made by the MEX file), else it is deleted
void release(mxArray* a, bool tomb) {
    for (mxArray* f : a->fvals)
        if (f) release(f, tomb);
    a->fvals.clear();
    std::free(a->raw);
    a->raw = nullptr;
    g_live.erase(a);
    if (tomb) g_dead.insert(a);
    else delete a;
}

uint64_t fnv(uint64_t h, const void* p, size_t n) {
    const unsigned char* b = (const unsigned char*)p;
    for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 1099511628211ull;
    return h;
}

uint64_t checksum(const mxArray* a, uint64_t h = 1469598103934665603ull) {
    const uint64_t head[4] = {(uint64_t)a->cls, a->is_struct, a->m, a->n};
    h = fnv(h, head, sizeof head);
    if (a->raw) h = fnv(h, a->data(), a->bytes);
    for (size_t i = 0; i < a->fvals.size(); ++i) {
        h = fnv(h, a->fnames[i].data(), a->fnames[i].size());
        h = fnv(h, &a->fvals[i], sizeof(mxArray*));
        if (a->fvals[i]) h = checksum(a->fvals[i], h);
    }
    return h;
}

void mark_input(mxArray* a, bool v) {
    a->input = v;
    for (mxArray* f : a->fvals)
        if (f) mark_input(f, v);
}

const mxArray* alive(const mxArray* a, const char* fn) {
    if (!a || !g_live.count(const_cast<mxArray*>(a))) {
        host_error("%s on %s", fn, !a ? "a NULL array" : g_dead.count(const_cast<mxArray*>(a)) ? "a destroyed array" : "a pointer that is no array");
        throw HostAbort();
    }
    return a;
}

void* typed(const mxArray* a, mxClassID want, const char* fn) {
    alive(a, fn);
    if (a->is_struct || a->cls != want) {
        host_error("%s on an array of class %d (%s)", fn, a->is_struct ? -1 : (int)a->cls, "an error under -R2018a");
        throw HostAbort();
    }
    return a->data();
}

void sweep_dead() {
    for (mxArray* a : g_dead) delete a;
    g_dead.clear();
}

}  // namespace

// ---- the MEX / matrix API of integration/mex_stub/mex.h -------------------------------------------------------
extern "C" {

void mexErrMsgIdAndTxt(const char* identifier, const char* fmt, ...) {
    char buf[2048];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    throw MexError{identifier ? identifier : "", buf};
}
void mexLock(void) { ++g_lock; }
int mexAtExit(void (*exit_fcn)(void)) {
    g_exit_fcn = exit_fcn;
    return 0;
}

bool mxIsDouble(const mxArray* pa) { return !alive(pa, "mxIsDouble")->is_struct && pa->cls == mxDOUBLE_CLASS; }
bool mxIsComplex(const mxArray* pa) { return alive(pa, "mxIsComplex"), false; }
bool mxIsStruct(const mxArray* pa) { return alive(pa, "mxIsStruct")->is_struct; }
bool mxIsChar(const mxArray* pa) { return !alive(pa, "mxIsChar")->is_struct && pa->cls == mxCHAR_CLASS; }
bool mxIsLogical(const mxArray* pa) { return !alive(pa, "mxIsLogical")->is_struct && pa->cls == mxLOGICAL_CLASS; }
bool mxIsEmpty(const mxArray* pa) { return alive(pa, "mxIsEmpty")->m == 0 || pa->n == 0; }
size_t mxGetM(const mxArray* pa) { return alive(pa, "mxGetM")->m; }
size_t mxGetN(const mxArray* pa) { return alive(pa, "mxGetN")->n; }
mwSize mxGetNumberOfDimensions(const mxArray* pa) { return alive(pa, "mxGetNumberOfDimensions"), 2; }
size_t mxGetNumberOfElements(const mxArray* pa) { return alive(pa, "mxGetNumberOfElements")->m * pa->n; }

double mxGetScalar(const mxArray* pa) {
    alive(pa, "mxGetScalar");
    if (pa->is_struct || pa->m * pa->n == 0) {  // (undefined in MATLAB: a struct, cell or empty array)
        host_error("mxGetScalar on %s", pa->is_struct ? "a struct" : "an empty array");
        throw HostAbort();
    }
    const unsigned char* d = pa->data();
    switch (pa->cls) {
        case mxLOGICAL_CLASS: return *(const bool*)d ? 1.0 : 0.0;
        case mxCHAR_CLASS: return (double)*(const uint16_t*)d;
        case mxDOUBLE_CLASS: return *(const double*)d;
        case mxSINGLE_CLASS: return (double)*(const float*)d;
        case mxINT16_CLASS: return (double)*(const int16_t*)d;
        case mxINT32_CLASS: return (double)*(const int32_t*)d;
        default: return 0.0;
    }
}
mxDouble* mxGetDoubles(const mxArray* pa) { return (mxDouble*)typed(pa, mxDOUBLE_CLASS, "mxGetDoubles"); }
mxInt16* mxGetInt16s(const mxArray* pa) { return (mxInt16*)typed(pa, mxINT16_CLASS, "mxGetInt16s"); }
mxLogical* mxGetLogicals(const mxArray* pa) { return (mxLogical*)typed(pa, mxLOGICAL_CLASS, "mxGetLogicals"); }

mxArray* mxGetField(const mxArray* pa, mwIndex index, const char* fieldname) {
    alive(pa, "mxGetField");
    if (!pa->is_struct || index != 0 || !fieldname) return nullptr;
    for (size_t i = 0; i < pa->fnames.size(); ++i)
        if (pa->fnames[i] == fieldname) return pa->fvals[i];
    return nullptr;
}

int mxGetString(const mxArray* pa, char* buf, mwSize buflen) {
    alive(pa, "mxGetString");
    if (!buf || buflen == 0) return 1;
    buf[0] = 0;
    if (pa->is_struct || pa->cls != mxCHAR_CLASS) return 1;
    const size_t len = pa->m * pa->n, k = len < buflen - 1 ? len : buflen - 1;
    const uint16_t* c = (const uint16_t*)pa->data();
    for (size_t i = 0; i < k; ++i) buf[i] = (char)c[i];
    buf[k] = 0;
    return len > buflen - 1 ? 1 : 0;
}

mxArray* mxCreateDoubleMatrix(mwSize m, mwSize n, mxComplexity flag) {
    if (flag != mxREAL) {
        host_error("complex arrays are not supported by this host");
        throw HostAbort();
    }
    return make(mxDOUBLE_CLASS, m, n);
}
mxArray* mxCreateDoubleScalar(double value) {
    mxArray* a = make(mxDOUBLE_CLASS, 1, 1);
    *(double*)a->data() = value;
    return a;
}
mxArray* mxCreateNumericMatrix(mwSize m, mwSize n, mxClassID classid, mxComplexity flag) {
    if (flag != mxREAL || classid == mxCHAR_CLASS || classid == mxLOGICAL_CLASS) {
        host_error("mxCreateNumericMatrix: class %d / complexity %d is not numeric real", (int)classid, (int)flag);
        throw HostAbort();
    }
    return make(classid, m, n);
}
mxArray* mxCreateStructMatrix(mwSize m, mwSize n, int nfields, const char** fieldnames) {
    if (m != 1 || n != 1) {
        host_error("this host makes 1 x 1 structs only");
        throw HostAbort();
    }
    mxArray* a = make_struct();
    for (int i = 0; i < nfields; ++i) {
        a->fnames.push_back(fieldnames[i]);
        a->fvals.push_back(nullptr);
    }
    return a;
}
void mxSetField(mxArray* pa, mwIndex index, const char* fieldname, mxArray* value) {
    alive(pa, "mxSetField");
    if (value) alive(value, "mxSetField (value)");
    if (!pa->is_struct || index != 0 || pa->input || (value && (value->input || value->owned))) {
        host_error("mxSetField: not a 1 x 1 struct of the caller's own, or a value that already belongs elsewhere");
        throw HostAbort();
    }
    for (size_t i = 0; i < pa->fnames.size(); ++i)
        if (pa->fnames[i] == fieldname) {
            pa->fvals[i] = value;  // (the previous value is not freed, as documented)
            if (value) value->owned = true;
            return;
        }
    host_error("mxSetField: no field '%s' (fields are fixed at creation)", fieldname);
    throw HostAbort();
}
mxArray* mxDuplicateArray(const mxArray* in) {
    alive(in, "mxDuplicateArray");
    if (in->is_struct) {
        mxArray* a = make_struct();
        a->fnames = in->fnames;
        for (const mxArray* f : in->fvals) {
            mxArray* c = f ? mxDuplicateArray(f) : nullptr;
            if (c) c->owned = true;
            a->fvals.push_back(c);
        }
        return a;
    }
    mxArray* a = make(in->cls, in->m, in->n);
    std::memcpy(a->data(), in->data(), in->bytes);
    return a;
}
void mxDestroyArray(mxArray* pa) {
    if (!pa) return;  // documented: NULL is ignored
    if (g_dead.count(pa)) return host_error("mxDestroyArray called twice on one array");
    if (!g_live.count(pa)) return host_error("mxDestroyArray on a pointer that is no array");
    if (pa->input) return host_error("mxDestroyArray on an input (prhs) array");
    if (pa->owned) return host_error("mxDestroyArray on a field of a struct");
    check_guards(pa, "seen at mxDestroyArray");
    release(pa, true);
}

// ---- the driver interface (ctypes) ------------------------------------------------------------------------------
// Arrays made here belong to the driver until mh_free; data is copied from caller memory (column-major).
mxArray* mh_make(int cls, size_t m, size_t n, const void* data) {
    try {
        mxArray* a = make((mxClassID)cls, m, n);
        if (data && a->bytes) std::memcpy(a->data(), data, a->bytes);
        return a;
    } catch (const HostAbort&) {
        return nullptr;
    }
}
mxArray* mh_make_struct(void) { return make_struct(); }
int mh_set_field(mxArray* s, const char* name, mxArray* v) {  // adds the field; the struct owns v from here on
    if (!s || !s->is_struct || !g_live.count(s) || (v && (!g_live.count(v) || v->owned))) return 1;
    s->fnames.push_back(name);
    s->fvals.push_back(v);
    if (v) v->owned = true;
    return 0;
}
void mh_free(mxArray* a) {
    if (a && g_live.count(a) && !a->owned) release(a, false);
}
int mh_class(const mxArray* a) { return a->is_struct ? -1 : (int)a->cls; }
size_t mh_m(const mxArray* a) { return a->m; }
size_t mh_n(const mxArray* a) { return a->n; }
size_t mh_bytes(const mxArray* a) { return a->bytes; }
const void* mh_data(const mxArray* a) { return a->raw ? a->data() : nullptr; }
int mh_nfields(const mxArray* a) { return (int)a->fnames.size(); }
const char* mh_field_name(const mxArray* a, int i) { return a->fnames[(size_t)i].c_str(); }
mxArray* mh_field_value(const mxArray* a, int i) { return a->fvals[(size_t)i]; }
size_t mh_guard_bytes(void) { return kGuard; }

// mexFunction(nlhs, plhs, nrhs, prhs).  Returns 0 = returned, 1 = mexErrMsgIdAndTxt (mh_err_id / mh_err_msg), 2 = the
// host stopped the call (see mh_error_*).  Results: mh_nout / mh_out, the driver's to mh_free.
int mh_call(int nlhs, int nrhs, mxArray** prhs) {
    for (mxArray* a : g_out) mh_free(a);
    g_out.clear();
    g_err_id.clear();
    g_err_msg.clear();
    g_created.clear();
    std::vector<uint64_t> sums;
    for (int i = 0; i < nrhs; ++i) {
        mark_input(prhs[i], true);
        sums.push_back(checksum(prhs[i]));
    }
    const int nret = nlhs > 1 ? nlhs : 1;
    std::vector<mxArray*> plhs((size_t)nret + kSlack, nullptr);
    g_in_call = true;
    g_status = 0;
    try {
        mexFunction(nlhs, plhs.data(), nrhs, const_cast<const mxArray**>(prhs));
    } catch (const MexError& e) {
        g_status = 1;
        g_err_id = e.id;
        g_err_msg = e.msg;
    } catch (const HostAbort&) {
        g_status = 2;
    } catch (const std::exception& e) {
        g_status = 2;
        host_error("C++ exception left mexFunction: %s", e.what());
    }
    g_in_call = false;
    for (int i = nret; i < nret + kSlack; ++i)
        if (plhs[(size_t)i]) host_error("plhs[%d] written, but only %d output(s) may be returned (nlhs = %d)", i, nret, nlhs);
    std::set<mxArray*> keep;
    if (g_status == 0)
        for (int i = 0; i < nret; ++i) {
            mxArray* a = plhs[(size_t)i];
            if (!a) {
                if (i < nlhs) host_error("plhs[%d] not assigned (nlhs = %d)", i, nlhs);
                continue;
            }
            if (g_dead.count(a)) host_error("plhs[%d] is an array the call destroyed", i);
            else if (!g_live.count(a)) host_error("plhs[%d] is no array", i);
            else if (a->input) host_error("plhs[%d] is an input array (it must be duplicated)", i);
            else if (a->owned || keep.count(a)) host_error("plhs[%d] is returned twice or is a field of a struct", i);
            else {
                keep.insert(a);
                g_out.push_back(a);
            }
        }
    for (int i = 0; i < nrhs; ++i) check_guards(prhs[i], "an input, after the call");
    for (mxArray* a : g_created)
        if (g_live.count(a) && !a->owned) check_guards(a, "an array the call created, after the call");
    for (mxArray* a : g_created)  // what MATLAB frees: temporaries, and everything after an error
        if (g_live.count(a) && !a->owned && !keep.count(a)) release(a, false);
    g_created.clear();
    for (int i = 0; i < nrhs; ++i) {
        if (checksum(prhs[i]) != sums[(size_t)i]) host_error("prhs[%d] was modified by the call (inputs are never modified)", i);
        mark_input(prhs[i], false);
    }
    sweep_dead();
    return g_status;
}
int mh_nout(void) { return (int)g_out.size(); }
mxArray* mh_out(int i) { return g_out[(size_t)i]; }
mxArray* mh_take_out(int i) {  // the driver takes the result over (it is no longer freed by the next mh_call)
    mxArray* a = g_out[(size_t)i];
    g_out[(size_t)i] = nullptr;
    return a;
}
const char* mh_err_id(void) { return g_err_id.c_str(); }
const char* mh_err_msg(void) { return g_err_msg.c_str(); }
int mh_lock_count(void) { return g_lock; }
int mh_has_exit_fcn(void) { return g_exit_fcn != nullptr; }
// "unload": what MATLAB does when the MEX file is cleared or MATLAB exits -- the exit function runs once, locks are void
int mh_unload(void) {
    void (*f)(void) = g_exit_fcn;
    g_exit_fcn = nullptr;
    g_lock = 0;
    if (!f) return 0;
    try {
        f();
    } catch (...) {
        host_error("the exit function raised");
        return 1;
    }
    return 0;
}
int mh_error_count(void) { return (int)g_errors.size(); }
const char* mh_error_get(int i) { return g_errors[(size_t)i].c_str(); }
void mh_error_clear(void) { g_errors.clear(); }
size_t mh_live_count(void) { return g_live.size(); }

}  // extern "C"
