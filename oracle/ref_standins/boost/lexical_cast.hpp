// functional stand-in (see ../README.md): boost::lexical_cast through a string stream
#pragma once
#include <sstream>
#include <stdexcept>
namespace boost {
template <class Target, class Source> Target lexical_cast(const Source &v)
{
    std::stringstream ss;
    Target t;
    if (!(ss << v) || !(ss >> t)) throw std::runtime_error("bad lexical cast");
    return t;
}
}  // namespace boost
