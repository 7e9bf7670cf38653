!  kkt_dev -- the reference's first driver problem (test/driver1.f90: the extended Rosenbrock function, odd variables
!  in [1, 100], even ones in [-100, 100], x0 = 3, factr = 1e7, pgtol = 1e-5) solved on device buffers with the
!  module's setulb_dev and the library's built-in objective, then the active set at the solution through the module's
!  report procedures: lbfgsb_kkt (status, multipliers, the summary) and lbfgsb_kkt_list (the indices of the rows at a
!  bound), all on hipMalloc'ed buffers.
!
!     kkt_dev [n [m [iterations]]]      defaults 25, 5, 0 (0: to convergence; k > 0: stop at iterate k --
!                                       at n = 1000, m = 7, k = 8 half of the variables sit on a bound)
!
!  Output: one "Iterate" line per iterate, the final task, then
!     KKT counts = <unbounded free lower upper fixed binding weak leaving outside>
!     KKT values = <max|proj g|  max|multiplier|  max distance outside  max|g| on free rows>
!     KKT active = <count> : <the first indices, 0-based>
      program kkt_dev

      use lbfgsb_module, wp => lbfgsp_wp
      use iso_c_binding
      use iso_fortran_env, only: output_unit

      implicit none

      interface
         function hipMalloc(ptr, nbytes) bind(C, name='hipMalloc') result(rc)
            import :: c_ptr, c_size_t, c_int
            type(c_ptr) :: ptr
            integer(c_size_t), value :: nbytes
            integer(c_int) :: rc
         end function hipMalloc
         function hipFree(ptr) bind(C, name='hipFree') result(rc)
            import :: c_ptr, c_int
            type(c_ptr), value :: ptr
            integer(c_int) :: rc
         end function hipFree
         function hipMemcpy(dst, src, nbytes, kind) bind(C, name='hipMemcpy') result(rc)
            import :: c_ptr, c_size_t, c_int
            type(c_ptr), value :: dst, src
            integer(c_size_t), value :: nbytes
            integer(c_int), value :: kind
            integer(c_int) :: rc
         end function hipMemcpy
         function hipMemset(dst, val, nbytes) bind(C, name='hipMemset') result(rc)
            import :: c_ptr, c_size_t, c_int
            type(c_ptr), value :: dst
            integer(c_int), value :: val
            integer(c_size_t), value :: nbytes
            integer(c_int) :: rc
         end function hipMemset
      end interface
      integer(c_int), parameter :: H2D = 1, D2H = 2
      integer, parameter    :: NSHOW = 8                                   ! indices printed

      integer               :: n, m, maxit, rc, i
      real(wp), parameter   :: factr = 1.0e7_wp, pgtol = 1.0e-5_wp
      character(len=60)     :: task, csave
      character(len=32)     :: arg
      logical               :: lsave(4)
      integer               :: isave(44)
      real(wp)              :: f, dsave(29)
      type(c_ptr)           :: ctx, dx, dg, dl, du, dnbd, dmult, dstatus, didx
      real(wp), allocatable, target :: hbuf(:)
      integer(c_int32_t), allocatable, target :: hnbd(:)
      integer(c_int64_t), target :: hidx(NSHOW)
      integer(c_int64_t)    :: cnt(LBFGSB_KKT_NCNT), nact, nshown
      real(c_double)        :: val(LBFGSB_KKT_NVAL)
      integer(c_size_t)     :: vbytes

      n = 25; m = 5; maxit = 0
      if (command_argument_count() >= 1) then
         call get_command_argument(1, arg); read (arg, *) n
      end if
      if (command_argument_count() >= 2) then
         call get_command_argument(2, arg); read (arg, *) m
      end if
      if (command_argument_count() >= 3) then
         call get_command_argument(3, arg); read (arg, *) maxit
      end if

      vbytes = int(n, c_size_t)*int(storage_size(1.0_wp)/8, c_size_t)
      call chk(hipMalloc(dx, vbytes), 'hipMalloc x')
      call chk(hipMalloc(dg, vbytes), 'hipMalloc g')
      call chk(hipMalloc(dl, vbytes), 'hipMalloc l')
      call chk(hipMalloc(du, vbytes), 'hipMalloc u')
      call chk(hipMalloc(dmult, vbytes), 'hipMalloc mult')
      call chk(hipMalloc(dstatus, int(n, c_size_t)), 'hipMalloc status')
      call chk(hipMalloc(didx, int(NSHOW, c_size_t)*8_c_size_t), 'hipMalloc idx')
      call chk(hipMalloc(dnbd, int(n, c_size_t)*4_c_size_t), 'hipMalloc nbd')
      call chk(hipMemset(dg, 0_c_int, vbytes), 'hipMemset g')
      allocate (hbuf(n))
      hbuf = 3.0_wp                                                        ! x0 = 3
      call chk(hipMemcpy(dx, c_loc(hbuf), vbytes, H2D), 'hipMemcpy x')
      do i = 1, n, 2                                                       ! odd variables: [1, 100]
         hbuf(i) = 1.0_wp
      end do
      do i = 2, n, 2                                                       ! even variables: [-100, 100]
         hbuf(i) = -100.0_wp
      end do
      call chk(hipMemcpy(dl, c_loc(hbuf), vbytes, H2D), 'hipMemcpy l')
      hbuf = 100.0_wp
      call chk(hipMemcpy(du, c_loc(hbuf), vbytes, H2D), 'hipMemcpy u')
      allocate (hnbd(n))
      hnbd = 2_c_int32_t
      call chk(hipMemcpy(dnbd, c_loc(hnbd), int(n, c_size_t)*4_c_size_t, H2D), 'hipMemcpy nbd')
      deallocate (hnbd)

      call lbfgsb_create(ctx, n, m, 0, rc)
      if (rc /= 0) then
         write (output_unit, '(2a)') ' lbfgsb_create failed: ', lbfgsb_error_message()
         error stop 1
      end if

      task = 'START'
      f = 0.0_wp
      do while (task(1:2) == 'FG' .or. task == 'NEW_X' .or. task == 'START')
         call setulb_dev(ctx, dx, dl, du, dnbd, f, dg, factr, pgtol, task, -1, csave, lsave, isave, dsave, rc)
         if (rc /= 0) then
            write (output_unit, '(2a)') ' setulb_dev failed: ', lbfgsb_error_message()
            error stop 1
         end if
         if (task(1:2) == 'FG') then
            call lbfgsb_objective(ctx, 1, dx, dg, rc, f)
            if (rc /= 0) error stop 2
         else if (task(1:5) == 'NEW_X') then
            write (output_unit, '(2(a,i5,4x),a,1p,d12.5,4x,a,1p,d12.5)') 'Iterate', isave(30), 'nfg =', isave(34), &
               'f =', f, '|proj g| =', dsave(13)
            if (maxit > 0 .and. isave(30) >= maxit) exit                   ! the active set of this iterate
         end if
      end do
      write (output_unit, '(2a)') ' task = ', trim(task)

      ! the active set at the last iterate: status and multipliers stay on the device, the summary comes to the host
      call lbfgsb_kkt(ctx, dx, dl, du, dnbd, dg, real(pgtol, c_double), c_null_ptr, dmult, dstatus, cnt, val, rc)
      if (rc /= 0) then
         write (output_unit, '(2a)') ' lbfgsb_kkt failed: ', lbfgsb_error_message()
         error stop 1
      end if
      ! the rows at a lower or an upper bound or fixed (codes 1, 2, 3: bits 2, 3, 4): the first NSHOW of them
      call lbfgsb_kkt_list(ctx, dstatus, 28, didx, int(NSHOW, c_int64_t), nact, rc)
      if (rc /= 0) then
         write (output_unit, '(2a)') ' lbfgsb_kkt_list failed: ', lbfgsb_error_message()
         error stop 1
      end if
      nshown = min(nact, int(NSHOW, c_int64_t))
      hidx = -1_c_int64_t
      if (nshown > 0) call chk(hipMemcpy(c_loc(hidx), didx, int(nshown, c_size_t)*8_c_size_t, D2H), 'hipMemcpy idx')
      write (output_unit, '(a,9(1x,i0))') 'KKT counts =', cnt
      write (output_unit, '(a,4(1x,es24.16))') 'KKT values =', val
      write (output_unit, '(a,1x,i0,1x,a,8(1x,i0))') 'KKT active =', nact, ':', hidx(1:nshown)

      call lbfgsb_destroy(ctx)
      rc = hipFree(dx); rc = hipFree(dg); rc = hipFree(dl); rc = hipFree(du)
      rc = hipFree(dmult); rc = hipFree(dstatus); rc = hipFree(didx); rc = hipFree(dnbd)

      contains

      subroutine chk(code, what)
      integer(c_int), intent(in) :: code
      character(len=*), intent(in) :: what
      if (code /= 0) then
         write (output_unit, '(3a,i0)') ' ', what, ' failed, hipError ', code
         error stop 3
      end if
      end subroutine chk

      end program kkt_dev
