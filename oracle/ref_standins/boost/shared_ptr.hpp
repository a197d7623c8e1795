// functional stand-in (see ../README.md): boost::shared_ptr as the standard one
#pragma once
#include <memory>
namespace boost {
template <class T> using shared_ptr = std::shared_ptr<T>;
}  // namespace boost
