// mock_mgk_sessions_line.cpp -- the stand-ins of the line smoothers (tests/mock_mgk_xchunkline.cpp and what it includes) and, in the same
// library, those that csrc/mg_fmg.c and csrc/mg_gmres.c name (tests/mock_mgk_fmg.cpp, mock_mgk_gmres.cpp), so that the line-smoother sessions
// of tools/stress_sessions_mock.py can call fmg, solve_fmg and solve_gmres on a line-smoother handle and be REFUSED by the product's own
// checks: a library without mg_fmg.c / mg_gmres.c has no such entry point to refuse anything.  Both chains include tests/mock_mgk.cpp, which
// guards itself against the second inclusion.  TEST INFRASTRUCTURE ONLY.
#include "mock_mgk_xchunkline.cpp"
#include "mock_mgk_fmg.cpp"
