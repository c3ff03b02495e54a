// replay_main.cpp -- a stand-alone program that replays recorded MEX calls through one shim + the test host, for a
// sanitizer pass over the shims' argument checks and error paths (plain host C++; nothing is loaded into an interpreter).
//
// The calls are the VALIDATION table of tests/test_mexhost.py, written out by tests/mexhost.py::dump_cases:
//     python -c "import sys; sys.path[:0] = ['.', 'tests']; import mexhost, test_mexhost as t; mexhost.dump_cases('cases.txt', t.VALIDATION)"
//     g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iintegration/mex_stub -Iinclude \
//         tests/mexhost/replay_main.cpp integration/<shim>.cpp tests/mexhost/mexhost.cpp \
//         -Lse_snmf_nat_amd -l:libsnmf_hip.so -Wl,-rpath,$PWD/se_snmf_nat_amd -o replay_<shim>
//     ./replay_<shim> <shim> cases.txt
// Every case must end in mexErrMsgIdAndTxt with the recorded id and without a host error; the exit status is the number
// of cases that did not.  Not run by pytest.
//
// File format, one token stream per case:  CASE <shim> <nlhs> <id> <nargs>  then per argument
//     A <class> <m> <n> <hex bytes | ->      or      S <nfields> { <name> <argument> }
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "mex.h"

extern "C" {
mxArray* mh_make(int cls, size_t m, size_t n, const void* data);
mxArray* mh_make_struct(void);
int mh_set_field(mxArray* s, const char* name, mxArray* v);
void mh_free(mxArray* a);
int mh_call(int nlhs, int nrhs, mxArray** prhs);
const char* mh_err_id(void);
const char* mh_err_msg(void);
int mh_error_count(void);
const char* mh_error_get(int i);
void mh_error_clear(void);
int mh_unload(void);
size_t mh_live_count(void);
int mh_nout(void);
mxArray* mh_take_out(int i);
}

static mxArray* read_arg(std::istream& in) {
    std::string kind;
    in >> kind;
    if (kind == "S") {
        int nf = 0;
        in >> nf;
        mxArray* s = mh_make_struct();
        for (int i = 0; i < nf; ++i) {
            std::string name;
            in >> name;
            mh_set_field(s, name.c_str(), read_arg(in));
        }
        return s;
    }
    int cls = 0;
    size_t m = 0, n = 0;
    std::string hex;
    in >> cls >> m >> n >> hex;
    std::vector<unsigned char> bytes;
    if (hex != "-")
        for (size_t i = 0; i + 1 < hex.size(); i += 2) bytes.push_back((unsigned char)std::stoi(hex.substr(i, 2), nullptr, 16));
    return mh_make(cls, m, n, bytes.empty() ? nullptr : bytes.data());
}

int main(int argc, char** argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: %s <shim name> <case file>\n", argv[0]);
        return 2;
    }
    std::ifstream in(argv[2]);
    std::string tok, shim, id;
    int ran = 0, bad = 0;
    while (in >> tok) {
        if (tok != "CASE") {
            std::fprintf(stderr, "malformed case file at '%s'\n", tok.c_str());
            return 2;
        }
        int nlhs = 0, nargs = 0;
        in >> shim >> nlhs >> id >> nargs;
        std::vector<mxArray*> args;
        for (int i = 0; i < nargs; ++i) args.push_back(read_arg(in));
        if (shim == argv[1]) {
            mh_error_clear();
            mxArray* none = nullptr;
            const int st = mh_call(nlhs, nargs, nargs ? args.data() : &none);
            ++ran;
            if (st != 1 || id != mh_err_id() || mh_error_count() != 0) {
                ++bad;
                std::fprintf(stderr, "case %d of %s: status %d id '%s' (want '%s') msg '%s'\n", ran, shim.c_str(), st, mh_err_id(), id.c_str(), mh_err_msg());
                for (int i = 0; i < mh_error_count(); ++i) std::fprintf(stderr, "  host error: %s\n", mh_error_get(i));
            }
            for (int i = 0; i < mh_nout(); ++i) mh_free(mh_take_out(i));
        }
        for (mxArray* a : args) mh_free(a);
    }
    mh_unload();
    if (mh_live_count() != 0) {
        ++bad;
        std::fprintf(stderr, "%zu arrays still alive at the end\n", mh_live_count());
    }
    std::printf("%s: %d cases replayed, %d wrong\n", argv[1], ran, bad);
    return bad;
}
