// ORACLE — test infrastructure only.  Deliberately empty: the reference's operator files include it and use nothing of it.
#pragma once
