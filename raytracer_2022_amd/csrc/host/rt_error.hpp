// rt_error.hpp — how the library reports a fault: Fail is thrown (RT_REQUIRE) and caught at the C ABI, which leaves its
// message in the thread-local error string behind rt_last_error() (include/rt2022.h). No HIP here: hip_owned.hpp adds RT_HIP.
#ifndef RT2022_RT_ERROR_HPP
#define RT2022_RT_ERROR_HPP
#include <string>
namespace rt2022 {
void set_error(const std::string &m);
struct Fail { int code; std::string msg; };
}
#define RT_REQUIRE(cond, code, msg) do { if (!(cond)) throw rt2022::Fail{code, msg}; } while (0)
#endif
