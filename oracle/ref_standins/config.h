// functional stand-in (see README.md): nothing to configure
