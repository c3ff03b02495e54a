// misbehave_mex.cpp -- a purpose-made WRONG mexFunction, so that tests/test_mexhost.py can see every check of the test
// host (tests/mexhost/mexhost.cpp) fire.  misbehave('what', ...): each command breaks one rule of the MEX contract.
// Every write stays inside memory this file's own arrays own (the guard zone belongs to the array's allocation).
#include <cstring>

#include "mex.h"

void mexFunction(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
    char cmd[32] = "";
    if (nrhs < 1 || mxGetString(prhs[0], cmd, sizeof cmd) != 0) mexErrMsgIdAndTxt("mis:usage", "misbehave('what', ...)");
    if (!std::strcmp(cmd, "ok")) {  // well-behaved: one result, one temporary left for the host to free
        plhs[0] = mxDuplicateArray(prhs[1]);
        mxCreateDoubleMatrix(3, 3, mxREAL);
    } else if (!std::strcmp(cmd, "guard")) {  // one element past the end of its own output
        plhs[0] = mxCreateDoubleMatrix(4, 1, mxREAL);
        mxGetDoubles(plhs[0])[4] = 1.0;
    } else if (!std::strcmp(cmd, "guard_before")) {  // one element before the start
        plhs[0] = mxCreateDoubleMatrix(4, 1, mxREAL);
        mxGetDoubles(plhs[0])[-1] = 1.0;
    } else if (!std::strcmp(cmd, "guard_temp")) {  // the same in a temporary that is destroyed before the call ends
        mxArray* t = mxCreateDoubleMatrix(2, 2, mxREAL);
        mxGetDoubles(t)[4] = 1.0;
        mxDestroyArray(t);
        plhs[0] = mxCreateDoubleScalar(0.0);
    } else if (!std::strcmp(cmd, "input")) {  // writes into prhs[1]
        const_cast<double*>(mxGetDoubles(prhs[1]))[0] += 1.0;
        plhs[0] = mxCreateDoubleScalar(0.0);
    } else if (!std::strcmp(cmd, "double_free")) {
        mxArray* t = mxCreateDoubleMatrix(2, 2, mxREAL);
        mxDestroyArray(t);
        mxDestroyArray(t);
        plhs[0] = mxCreateDoubleScalar(0.0);
    } else if (!std::strcmp(cmd, "free_input")) {
        mxDestroyArray(const_cast<mxArray*>(prhs[1]));
        plhs[0] = mxCreateDoubleScalar(0.0);
    } else if (!std::strcmp(cmd, "return_destroyed")) {
        plhs[0] = mxCreateDoubleMatrix(2, 2, mxREAL);
        mxDestroyArray(plhs[0]);
    } else if (!std::strcmp(cmd, "return_input")) {
        plhs[0] = const_cast<mxArray*>(prhs[1]);
    } else if (!std::strcmp(cmd, "extra_plhs")) {  // a second output nobody asked for
        plhs[0] = mxCreateDoubleScalar(0.0);
        plhs[nlhs > 1 ? nlhs : 1] = mxCreateDoubleScalar(1.0);
    } else if (!std::strcmp(cmd, "wrong_type")) {  // -R2018a: mxGetDoubles on a logical is an error
        plhs[0] = mxCreateDoubleScalar(mxGetDoubles(prhs[1])[0]);
    } else if (!std::strcmp(cmd, "error_after_create")) {  // arrays alive when the error leaves the call
        mxCreateDoubleMatrix(5, 5, mxREAL);
        plhs[0] = mxCreateDoubleMatrix(2, 2, mxREAL);
        mexErrMsgIdAndTxt("mis:boom", "value %d and '%s'", 42, "text");
    } else if (!std::strcmp(cmd, "scalar")) {  // mxGetScalar of prhs[1]
        plhs[0] = mxCreateDoubleScalar(mxGetScalar(prhs[1]));
    } else if (!std::strcmp(cmd, "string")) {  // mxGetString of prhs[1] into a buffer of prhs[2] bytes: [status, length read]
        char buf[64];
        size_t n = (size_t)mxGetScalar(prhs[2]);
        const int st = mxGetString(prhs[1], buf, n < sizeof buf ? n : sizeof buf);
        plhs[0] = mxCreateDoubleMatrix(1, 2, mxREAL);
        mxGetDoubles(plhs[0])[0] = st;
        mxGetDoubles(plhs[0])[1] = (double)std::strlen(buf);
    } else if (!std::strcmp(cmd, "field")) {  // [field present, isempty(field)] of prhs[1].<prhs[2]>
        char name[32];
        mxGetString(prhs[2], name, sizeof name);
        const mxArray* f = mxGetField(prhs[1], 0, name);
        plhs[0] = mxCreateDoubleMatrix(1, 2, mxREAL);
        mxGetDoubles(plhs[0])[0] = f != nullptr;
        mxGetDoubles(plhs[0])[1] = f ? mxIsEmpty(f) : -1;
    } else if (!std::strcmp(cmd, "make")) {  // zero-filled arrays of the creation calls, returned as a struct
        const char* names[4] = {"d", "i16", "i32", "s"};
        plhs[0] = mxCreateStructMatrix(1, 1, 4, names);
        mxSetField(plhs[0], 0, "d", mxCreateDoubleMatrix(2, 3, mxREAL));
        mxSetField(plhs[0], 0, "i16", mxCreateNumericMatrix(3, 1, mxINT16_CLASS, mxREAL));
        mxSetField(plhs[0], 0, "i32", mxCreateNumericMatrix(1, 2, mxINT32_CLASS, mxREAL));
        mxSetField(plhs[0], 0, "s", mxCreateNumericMatrix(2, 2, mxSINGLE_CLASS, mxREAL));
    } else if (!std::strcmp(cmd, "lock")) {
        mexLock();
        plhs[0] = mxCreateDoubleScalar(0.0);
    } else {
        mexErrMsgIdAndTxt("mis:cmd", "unknown command '%s'", cmd);
    }
}
